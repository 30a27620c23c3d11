"""Tensor-level wrappers over the C-ABI (device memory is borrowed from torch).

Everything here is a thin marshalling layer: shape checks, output allocation,
one C call.  No arithmetic happens in Python.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_PRELU, ACT_RELU, STORE_BF16, STORE_F16, STORE_NONE, ConvDesc,  # noqa: F401
                   ConvIO, check, current_stream, ptr)

LEAKY_SLOPE = 0.01


def _dev_f32(t, name, contiguous=True, shape=None):
    """None passes (optional arguments); otherwise a float32 GPU tensor, contiguous unless told otherwise, and of
    exactly ``shape`` when one is given."""
    if t is None:
        return
    if not (t.is_cuda and t.dtype == torch.float32 and (t.is_contiguous() or not contiguous)):
        raise ValueError(f"{name}: expected a contiguous float32 tensor on the GPU, got "
                         f"{t.dtype} {t.device} contiguous={t.is_contiguous()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def _dev_mask(mask, y):
    """An optional elementwise mask of the encoder passes: float32 on the GPU, contiguous, one value per element of ``y``."""
    _dev_f32(mask, "mask")
    if mask is not None and mask.numel() != y.numel():
        raise ValueError(f"mask: expected {y.numel()} elements (the shape {tuple(y.shape)}), got {tuple(mask.shape)}")


def _dense2d(t, name):
    """A contiguous [R,C] float32 GPU tensor (the kernel hard-codes pitch C).  Returns (rows, cols)."""
    _dev_f32(t, name)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D [R, C] tensor, got shape {tuple(t.shape)}")
    return t.shape[0], t.shape[1]


def _rows(t, name):
    """Accept a [R,C] tensor that is dense or a column slice of a wider row-major buffer.
    Returns (rows, cols, pitch)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
        raise ValueError(f"{name}: expected a 2-D float32 GPU tensor with unit column stride")
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _empty(shape, like):
    return torch.empty(shape, device=like.device, dtype=torch.float32)


def conv_kpad(kh, kw, cin):
    return _lib.load().cer_conv_kpad(kh, kw, cin)


def pack_conv_weight(w_oihw, out_scale=None, flip=False, transpose=False):
    """[Cout,Cin,KH,KW] -> [Cout,Kpad] with k = (kh*KW+kw)*Cin + c, BN scale folded;
    ``transpose`` gives the data-gradient filter [Cin, Kpad(KH,KW,Cout)]."""
    _dev_f32(w_oihw, "w_oihw")
    _dev_f32(out_scale, "out_scale")
    cout, cin, kh, kw = w_oihw.shape
    rows, inner = (cin, cout) if transpose else (cout, cin)
    out = _empty((rows, conv_kpad(kh, kw, inner)), w_oihw)
    check(_lib.load().cer_pack_conv_weight(ptr(w_oihw), ptr(out_scale), ptr(out), cout, cin, kh, kw,
                                           1 if flip else 0, 1 if transpose else 0, current_stream()),
          "cer_pack_conv_weight")
    return out


def _conv_desc(n, h, w, cin, cout, kh, kw, *, stride=1, dil=(1, 1), pad=(0, 0), out_hw=None, res_stride=1, Hr=0, Wr=0,
               act1=ACT_NONE, act2=ACT_NONE, slope=LEAKY_SLOPE, split_k=1, tile=0, x_nchw=False, x_ld=0, y_ld=0,
               storage=STORE_NONE, x_s2d=False, y_s2d=False, kpad=None):
    """The cer_conv_desc of one conv: (n, h, w, cin) is the input TENSOR's shape, so under ``x_s2d`` (a space-to-depth
    tensor) the conv's own input is [n, 2h, 2w, cin/4].  ``kpad``: the packed weight's K, checked against ``conv_kpad``
    (the only library call in here; without it this is plain ctypes)."""
    if x_s2d:
        if cin % 4:
            raise ValueError("a space-to-depth input has 4 * Cin channels")
        h, w, cin = 2 * h, 2 * w, cin // 4
    if kpad is not None and kpad != conv_kpad(kh, kw, cin):
        raise ValueError(f"packed weight has K={kpad}, expected {conv_kpad(kh, kw, cin)}")
    if out_hw is None:
        ho = (h + 2 * pad[0] - dil[0] * (kh - 1) - 1) // stride + 1
        wo = (w + 2 * pad[1] - dil[1] * (kw - 1) - 1) // stride + 1
    else:
        ho, wo = out_hw
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = n, h, w, cin, ho, wo, cout
    d.KH, d.KW, d.stride, d.dil_h, d.dil_w, d.pad_t, d.pad_l = kh, kw, stride, dil[0], dil[1], pad[0], pad[1]
    d.x_nchw, d.res_stride, d.Hr, d.Wr = int(x_nchw), res_stride, Hr, Wr
    d.act1, d.act2, d.slope, d.split_k, d.tile = act1, act2, slope, split_k, tile
    d.x_ld, d.y_ld, d.storage, d.x_s2d, d.y_s2d = x_ld, y_ld, storage, int(x_s2d), int(y_s2d)
    return d


def _res_kind(res, name, split=False, n16=None):
    """An optional residual as (fp32 tensor, hi or narrow plane, lo plane, Hr, Wr): an fp32 tensor always passes, a Split
    where ``split`` is set (bf16x3 family), a narrow tensor of dtype ``n16`` where that is given (narrow family)."""
    if res is None:
        return None, None, None, 0, 0
    hr, wr = res.shape[1], res.shape[2]
    if split and isinstance(res, Split):
        _dev_bf16(res.hi, f"{name}.hi")
        return None, res.hi, res.lo, hr, wr
    if n16 is not None and res.dtype != torch.float32:
        _dev_n16(res, name, n16)
        return None, res, None, hr, wr
    _dev_f32(res, name)
    return res, None, None, hr, wr


def _conv_epilogue(d, io, bias, alpha, bias9, residual, split=False, n16=None):
    """What the three conv wrappers check and marshal alike: the per-output-channel vectors, ``bias9`` and the residual
    (kinds as in ``_res_kind``), written into ``d`` / ``io``."""
    n, cout = d.N, d.Cout
    for t, nme in ((bias, "bias"), (alpha, "alpha")):
        _dev_f32(t, nme)
        if t is not None:
            if t.numel() != cout:
                raise ValueError(f"{nme} has {t.numel()} elements, expected {cout}")
            setattr(io, nme, t.data_ptr())
    if bias9 is not None:
        _dev_f32(bias9, "bias9")
        if tuple(bias9.shape) != (9, cout):
            raise ValueError("bias9 must be [9, Cout]")
        io.bias9 = bias9.data_ptr()
    if residual is not None:
        if residual.shape[0] != n or residual.shape[3] != cout:
            raise ValueError(f"residual shape {tuple(residual.shape)} does not match N={n}, Cout={cout}")
        r32, hi, lo, d.Hr, d.Wr = _res_kind(residual, "residual", split, n16)
        for name, t in (("residual", r32), ("res_hi", hi), ("res_lo", lo)):
            if t is not None:
                setattr(io, name, t.data_ptr())


def _next_affine_out(io, res, next_affine, shape, device):
    """The second Split output, out * s2 + t2, of the kernels with split outputs: allocated into ``res['next']``."""
    s2, t2 = next_affine
    _dev_f32(s2, "s2")
    _dev_f32(t2, "t2")
    res["next"] = Split.empty(shape, device)
    io.s2, io.t2 = s2.data_ptr(), t2.data_ptr()
    io.y2_hi, io.y2_lo = res["next"].hi.data_ptr(), res["next"].lo.data_ptr()


# bench.py sets this to a list to time every bf16x3 / narrow conv launch with HIP events on the launch stream:
# (kernel variant id, algorithmic FLOPs, start event, end event, algorithmic bytes)
CONV_TRACE = None


def _conv_run(d, io, family, device, trace=None, want_stats=False):
    """The one launch of every conv wrapper (cer_conv2d_run).  Allocates the split-K workspace and, with ``want_stats``,
    the [tiles,2,Cout] partial sums of kernel family ``family`` (0 fp32, 1 bf16x3, 2 narrow), which it returns.  ``trace``
    = (name of the family's tile query, algorithmic bytes): the launch enters ``CONV_TRACE`` when that is a list."""
    lib = _lib.load()
    stats = None
    if want_stats:
        stats = torch.empty((lib.cer_conv2d_stats_tiles(ctypes.byref(d), family), 2, d.Cout), device=device, dtype=torch.float32)
        io.stats = stats.data_ptr()
    ws_bytes = lib.cer_conv2d_workspace_bytes(ctypes.byref(d))
    ws = torch.empty((ws_bytes // 4,), device=device, dtype=torch.float32) if ws_bytes else None
    traced = trace is not None and CONV_TRACE is not None
    if traced:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib.cer_conv2d_run(ctypes.byref(d), ctypes.byref(io), ptr(ws), ws_bytes, current_stream()), "cer_conv2d_run")
    if traced:
        e1.record()
        tile_query, nbytes = trace
        CONV_TRACE.append((getattr(lib, tile_query)(ctypes.byref(d)), 2.0 * d.N * d.Ho * d.Wo * d.Cout * d.Cin * d.KH * d.KW,
                           e0, e1, nbytes))
    return stats


def conv2d(x, w_packed, kh, kw, *, stride=1, dil=(1, 1), pad=(0, 0), out_hw=None, in_scale=None,
           in_shift=None, bias=None, alpha=None, residual=None, res_stride=1, mask=None, act1=ACT_NONE,
           act2=ACT_NONE, slope=LEAKY_SLOPE, split_k=1, x_nchw=False, tile=0, out=None, aux=None, x_ld=0, y_ld=0,
           x_shape=None, want_stats=False, out_split=False, next_affine=None, want_f32=True, out_n16=None):
    """y[N,Ho,Wo,Cout] = act2(mask*act1(conv(affine(x), w)+bias) + residual).  x is NHWC
    (or NCHW with ``x_nchw`` on the small-Cin path).  ``x_shape`` = (N,H,W,Cin) overrides
    x.shape when x is a column slice (then ``x_ld`` is its row pitch).  Returns y, or (y, stats) with ``want_stats``;
    with ``out_split`` / ``next_affine`` (Split outputs: feeds the bf16x3 layers) or ``out_n16`` (a narrow output of that
    dtype: the Cin = 3 stem of the narrow encoder) a dict with 'y', 'stats' and 'split' / 'next' / 'n16'."""
    for t, n in ((w_packed, "w"), (in_scale, "in_scale"), (in_shift, "in_shift"), (mask, "mask"), (aux, "aux")):
        _dev_f32(t, n)
    _dev_f32(x, "x", contiguous=(x_ld == 0))
    if x_shape is not None:
        n, h, w, cin = x_shape
    elif x_nchw:
        n, cin, h, w = x.shape
    else:
        n, h, w, cin = x.shape
    cout = w_packed.shape[0]
    if out_n16 is not None and (out_split or next_affine is not None):
        raise ValueError("out_n16 excludes the split outputs")
    d = _conv_desc(n, h, w, cin, cout, kh, kw, stride=stride, dil=dil, pad=pad, out_hw=out_hw, res_stride=res_stride,
                   act1=act1, act2=act2, slope=slope, split_k=split_k, tile=tile, x_nchw=x_nchw, x_ld=x_ld, y_ld=y_ld,
                   storage=STORE_NONE if out_n16 is None else storage_of(out_n16), kpad=w_packed.shape[1])
    shape = (n, d.Ho, d.Wo, cout)
    for t, nme in ((in_scale, "in_scale"), (in_shift, "in_shift")):
        if t is not None and t.numel() != cin:
            raise ValueError(f"{nme} has {t.numel()} elements, expected {cin}")
    for t, nme in ((mask, "mask"), (aux, "aux")):
        if t is not None and t.numel() != n * d.Ho * d.Wo * cout:
            raise ValueError(f"{nme} must have the output's shape")
    if out is None and want_f32:
        if y_ld:
            raise ValueError("y_ld needs an explicit out buffer")
        out = _empty(shape, x)
    elif out is not None:
        _dev_f32(out, "out", contiguous=(y_ld == 0))
    io = ConvIO()
    io.x, io.w = x.data_ptr(), w_packed.data_ptr()
    for name, t in (("in_scale", in_scale), ("in_shift", in_shift), ("mask", mask), ("y", out), ("aux", aux)):
        if t is not None:
            setattr(io, name, t.data_ptr())
    _conv_epilogue(d, io, bias, alpha, None, residual)
    res = {"y": out, "stats": None}
    if out_n16 is not None:
        res["n16"] = torch.empty(shape, device=x.device, dtype=out_n16)
        io.y_hi = res["n16"].data_ptr()
    if out_split:
        res["split"] = Split.empty(shape, x.device)
        io.y_hi, io.y_lo = res["split"].hi.data_ptr(), res["split"].lo.data_ptr()
    if next_affine is not None:
        _next_affine_out(io, res, next_affine, shape, x.device)
    res["stats"] = _conv_run(d, io, 0, x.device, want_stats=want_stats)  # no trace: the fp32 convs stay out of CONV_TRACE
    if len(res) > 2:
        return res
    return (out, res["stats"]) if want_stats else out


class Split:
    """A tensor carried as two bf16 planes: value = hi + lo (hi = bf16(v), lo = bf16(v - hi))."""
    __slots__ = ("hi", "lo")

    def __init__(self, hi, lo):
        self.hi, self.lo = hi, lo

    @property
    def shape(self):
        return self.hi.shape

    def float(self):
        return self.hi.float() + self.lo.float()

    def view(self, *shape):
        return Split(self.hi.view(*shape), self.lo.view(*shape))

    @staticmethod
    def empty(shape, device):
        return Split(torch.empty(shape, device=device, dtype=torch.bfloat16),
                     torch.empty(shape, device=device, dtype=torch.bfloat16))


def split_bf16(x, scale=None, shift=None):
    """fp32 tensor -> Split (round-to-nearest-even on both parts), optionally after the per-channel
    affine x*scale[c]+shift[c] over the last (channel) axis."""
    _dev_f32(x, "x")
    _dev_f32(scale, "scale", shape=x.shape[-1:])
    _dev_f32(shift, "shift", shape=x.shape[-1:])
    out = Split.empty(x.shape, x.device)
    c = x.shape[-1] if scale is not None else 0
    check(_lib.load().cer_split_bf16(ptr(x), ptr(scale), ptr(shift), c, ptr(out.hi), ptr(out.lo), x.numel(),
                                     current_stream()), "cer_split_bf16")
    return out


def _dev_bf16(t, name):
    if t is not None and not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous bfloat16 GPU tensor")


def conv2d_b3(x, w, kh, kw, *, stride=1, dil=(1, 1), pad=(0, 0), out_hw=None, bias=None, alpha=None, residual=None,
              res_stride=1, act1=ACT_NONE, act2=ACT_NONE, slope=LEAKY_SLOPE, split_k=1, tile=0, out_f32=False,
              out_split=True, next_affine=None, want_stats=False, bias9=None, x_s2d=False, y_s2d=False):
    """bf16x3 convolution.  x, w: Split tensors (x NHWC [N,H,W,Cin], w [Cout,Kpad]); residual: Split
    or fp32 tensor.  Returns a dict with the requested outputs: 'y' (fp32), 'split' (Split), 'next'
    (Split of out*s2+t2 when ``next_affine=(s2, t2)``), 'stats'.
    ``y_s2d``: the Split output is stored space-to-depth, [N, Ho/2, Wo/2, 4*Cout] (``space_to_depth`` is the torch
    statement of the layout); ``x_s2d``: x is such a tensor (of the [N, 2*x.shape[1], 2*x.shape[2], x.shape[3]/4] input of
    this 3x3 / stride 2 / pad 1 conv) and w went through ``pack_s2d_weight``."""
    for t, n in ((x.hi, "x.hi"), (x.lo, "x.lo"), (w.hi, "w.hi"), (w.lo, "w.lo")):
        _dev_bf16(t, n)
    d = _conv_desc(*x.shape, w.shape[0], kh, kw, stride=stride, dil=dil, pad=pad, out_hw=out_hw, res_stride=res_stride, act1=act1,
                   act2=act2, slope=slope, split_k=split_k, tile=tile, x_s2d=x_s2d, y_s2d=y_s2d, kpad=w.shape[1])
    n, ho, wo, cout = d.N, d.Ho, d.Wo, d.Cout
    io = ConvIO()
    io.x_hi, io.x_lo, io.w_hi, io.w_lo = x.hi.data_ptr(), x.lo.data_ptr(), w.hi.data_ptr(), w.lo.data_ptr()
    _conv_epilogue(d, io, bias, alpha, bias9, residual, split=True)
    res = {}
    dev = x.hi.device
    if out_f32:
        res["y"] = torch.empty((n, ho, wo, cout), device=dev, dtype=torch.float32)
        io.y = res["y"].data_ptr()
    if out_split:
        res["split"] = Split.empty((n, ho // 2, wo // 2, 4 * cout) if y_s2d else (n, ho, wo, cout), dev)
        io.y_hi, io.y_lo = res["split"].hi.data_ptr(), res["split"].lo.data_ptr()
    if next_affine is not None:
        _next_affine_out(io, res, next_affine, (n, ho, wo, cout), dev)
    trace = None
    if CONV_TRACE is not None:
        # algorithmic bytes: split input (4 B/elt) + every output tensor written + split weights + residual read
        nout = n * ho * wo * cout
        nbytes = 4.0 * n * d.H * d.W * d.Cin + 4.0 * nout * (int(out_f32) + int(out_split) + int(next_affine is not None)) + \
            4.0 * cout * d.Cin * kh * kw + (4.0 * nout if residual is not None else 0.0)
        trace = ("cer_conv2d_b3_tile", nbytes)
    stats = _conv_run(d, io, 1, dev, trace, want_stats)
    if want_stats:
        res["stats"] = stats
    return res


def stem_conv(x, w, scale=None, shift=None, alpha=None, out=None, want_stats=False):
    """IR-50 input layer on the vector ALUs (cer_stem_conv3x3).  x [N,3,H,W] fp32 (NCHW), w the packed [64, Kpad] weight.
    ``out`` = None: the statistics pass -- returns the [rows,2,64] partial sums of the RAW conv result.  Otherwise ``out`` is
    "f32", "split", torch.bfloat16 or torch.float16 and the result is ``prelu(conv*scale+shift, alpha)`` in that storage,
    returned as a dict with 'y' / 'split' / 'n16' and (``want_stats``) 'stats' of that output."""
    _dev_f32(x, "x")
    _dev_f32(w, "w")
    for t, nme in ((scale, "scale"), (shift, "shift"), (alpha, "alpha")):
        _dev_f32(t, nme)
    n, c, h, wd = x.shape
    if c != 3 or w.shape[0] != 64:
        raise ValueError("stem_conv is the 3 -> 64 input layer")
    lib = _lib.load()
    stats = _empty((lib.cer_stem_conv3x3_stats_rows(n, h), 2, 64), x) if (want_stats or out is None) else None
    res, y, hi, lo, storage = {}, None, None, None, STORE_NONE
    if out == "f32":
        res["y"] = y = torch.empty((n, h, wd, 64), device=x.device, dtype=torch.float32)
    elif out == "split":
        res["split"] = Split.empty((n, h, wd, 64), x.device)
        hi, lo = res["split"].hi, res["split"].lo
    elif out is not None:
        storage = storage_of(out)
        res["n16"] = hi = torch.empty((n, h, wd, 64), device=x.device, dtype=out)
    check(lib.cer_stem_conv3x3(ptr(x), ptr(w), w.shape[1], ptr(scale), ptr(shift), ptr(alpha), ptr(y), ptr(hi), ptr(lo), storage,
                               ptr(stats), n, h, wd, current_stream()), "cer_stem_conv3x3")
    if out is None:
        return stats
    if want_stats:
        res["stats"] = stats
    return res


def _tile_query(query, n, h, w, cin, cout, kh, kw, stride, pad, x_s2d):
    d = _conv_desc(n, h, w, cin, cout, kh, kw, stride=stride, pad=pad)
    d.x_s2d = int(x_s2d)  # (n, h, w, cin) is the conv's own input here, not the space-to-depth tensor
    return getattr(_lib.load(), query)(ctypes.byref(d))


def conv2d_b3_tile(n, h, w, cin, cout, kh, kw, stride, pad, x_s2d=False):
    """The bf16x3 kernel variant ``conv2d_b3`` would launch for this conv (cer_conv2d_b3_tile)."""
    return _tile_query("cer_conv2d_b3_tile", n, h, w, cin, cout, kh, kw, stride, pad, x_s2d)


def conv2d_n16_tile(n, h, w, cin, cout, kh, kw, stride, pad, x_s2d=False):
    """The narrow kernel variant ``conv2d_n16`` would launch for this conv (cer_conv2d_n16_tile)."""
    return _tile_query("cer_conv2d_n16_tile", n, h, w, cin, cout, kh, kw, stride, pad, x_s2d)


# the window / patch kernels: their epilogues can store space-to-depth
S2D_PRODUCER_TILES = (53, 56, 58, 59)
S2D_PRODUCER_TILES_N16 = (71, 72, 73, 76, 77, 78, 79)


def s2d_k_order(cin, device, chunk=32):
    """K-column order of an ``x_s2d`` conv's weights (cer_conv_s2d_k_order) as an index tensor; chunk = channels per kernel
    step: 32 (bf16x3) or 64 (narrow)."""
    order = (ctypes.c_int32 * (9 * cin))()
    check(_lib.load().cer_conv_s2d_k_order(cin, chunk, order), "cer_conv_s2d_k_order")
    return torch.tensor(list(order), dtype=torch.long, device=device)


def pack_s2d_weight(w, cin, chunk=None):
    """Packed 3x3 weights [Cout, 9*Cin] (Split, or a narrow / fp32 plane) -> the same columns in the step order of the
    space-to-depth stride-2 kernel (chunk: 32 for Split operands, 64 for a narrow plane)."""
    if isinstance(w, Split):
        idx = s2d_k_order(cin, w.hi.device, chunk or 32)
        return Split(w.hi.index_select(1, idx).contiguous(), w.lo.index_select(1, idx).contiguous())
    return w.index_select(1, s2d_k_order(cin, w.device, chunk or 64)).contiguous()


def space_to_depth(x):
    """[N, H, W, C] -> [N, H/2, W/2, 4C] with channel blocks ordered P11 | P10 | P01 | P00 (block = 3 - 2*(row & 1) - (col & 1)):
    the torch statement of the layout ``y_s2d`` stores and ``x_s2d`` reads (tests; the product path never makes this copy)."""
    if isinstance(x, Split):
        return Split(space_to_depth(x.hi), space_to_depth(x.lo))
    return torch.cat([x[:, 1::2, 1::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 0::2, 0::2]], dim=3).contiguous()


# ------------------------------------------------------------------ narrow storage (one bf16 / half plane per tensor)
def storage_of(dtype):
    """torch dtype -> cer_storage of the narrow kernels."""
    if dtype == torch.bfloat16:
        return STORE_BF16
    if dtype == torch.float16:
        return STORE_F16
    raise ValueError(f"narrow storage is torch.bfloat16 or torch.float16, got {dtype}")


def _dev_n16(t, name, dtype=None):
    if t is None:
        return
    if not (t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) and t.is_contiguous()) or (dtype is not None and t.dtype != dtype):
        raise ValueError(f"{name}: expected a contiguous {dtype or 'bfloat16/float16'} GPU tensor, got {t.dtype} {t.device}")


def to_n16(x, dtype, scale=None, shift=None):
    """fp32 tensor -> narrow tensor (round-to-nearest-even), optionally after x*scale[c]+shift[c] over the last axis."""
    _dev_f32(x, "x")
    _dev_f32(scale, "scale", shape=x.shape[-1:])
    _dev_f32(shift, "shift", shape=x.shape[-1:])
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    c = x.shape[-1] if scale is not None else 0
    check(_lib.load().cer_to_n16(ptr(x), ptr(scale), ptr(shift), c, ptr(out), x.numel(), storage_of(dtype), current_stream()),
          "cer_to_n16")
    return out


def from_n16(x):
    _dev_n16(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    check(_lib.load().cer_from_n16(ptr(x), ptr(out), x.numel(), storage_of(x.dtype), current_stream()), "cer_from_n16")
    return out


def conv2d_n16(x, w, kh, kw, *, stride=1, dil=(1, 1), pad=(0, 0), out_hw=None, bias=None, alpha=None, residual=None,
               res_stride=1, act1=ACT_NONE, act2=ACT_NONE, slope=LEAKY_SLOPE, split_k=1, tile=0, out_f32=False,
               out_n16=True, want_stats=False, bias9=None, x_s2d=False, y_s2d=False):
    """Narrow convolution: x [N,H,W,Cin] and w [Cout,Kpad] are bf16 / float16 tensors of the same dtype (one MFMA per
    product, fp32 accumulate); residual: narrow or fp32.  Returns a dict with 'n16' (narrow output), 'y' (fp32), 'stats'.
    ``x_s2d`` / ``y_s2d``: space-to-depth input / narrow output, as in ``conv2d_b3`` (weights: ``pack_s2d_weight(w, cin, 64)``)."""
    _dev_n16(x, "x")
    _dev_n16(w, "w", x.dtype)
    d = _conv_desc(*x.shape, w.shape[0], kh, kw, stride=stride, dil=dil, pad=pad, out_hw=out_hw, res_stride=res_stride, act1=act1,
                   act2=act2, slope=slope, split_k=split_k, tile=tile, storage=storage_of(x.dtype), x_s2d=x_s2d, y_s2d=y_s2d,
                   kpad=w.shape[1])
    n, ho, wo, cout = d.N, d.Ho, d.Wo, d.Cout
    io = ConvIO()
    io.x_hi, io.w_hi = x.data_ptr(), w.data_ptr()
    _conv_epilogue(d, io, bias, alpha, bias9, residual, n16=x.dtype)
    res = {}
    dev = x.device
    if out_f32:
        res["y"] = torch.empty((n, ho, wo, cout), device=dev, dtype=torch.float32)
        io.y = res["y"].data_ptr()
    if out_n16:
        res["n16"] = torch.empty((n, ho // 2, wo // 2, 4 * cout) if y_s2d else (n, ho, wo, cout), device=dev, dtype=x.dtype)
        io.y_hi = res["n16"].data_ptr()
    trace = None
    if CONV_TRACE is not None:
        # algorithmic bytes: narrow input + every output tensor written + narrow weights + residual read
        nout = n * ho * wo * cout
        nbytes = 2.0 * n * d.H * d.W * d.Cin + nout * (4.0 * int(out_f32) + 2.0 * int(out_n16)) + 2.0 * cout * d.Cin * kh * kw + \
            (0.0 if residual is None else (4.0 if residual.dtype == torch.float32 else 2.0) * nout)
        trace = ("cer_conv2d_n16_tile", nbytes)
    stats = _conv_run(d, io, 2, dev, trace, want_stats)
    if want_stats:
        res["stats"] = stats
    return res


def _bn_apply_args(y, scale, shift, alpha, res, res_scale, res_shift, mask, split=False, n16=None):
    """What the three ``bn_apply`` wrappers check alike: the (C,) vectors, the mask and that the residual has the images and
    channels of ``y`` (the kernel indexes it with both); returns ``_res_kind(res)``."""
    n, c = y.shape[0], y.shape[3]
    for t, nme in ((scale, "scale"), (shift, "shift"), (alpha, "alpha"), (res_scale, "res_scale"), (res_shift, "res_shift")):
        _dev_f32(t, nme, shape=(c,))
    _dev_mask(mask, y)
    if res is not None and (len(res.shape) != 4 or res.shape[0] != n or res.shape[3] != c):
        raise ValueError(f"res shape {tuple(res.shape)} does not match N={n}, C={c}")
    return _res_kind(res, "res", split, n16)


def bn_apply_nhwc_n16(y, scale, shift, dtype=None, alpha=None, res=None, res_stride=1, res_scale=None, res_shift=None, mask=None,
                      want_stats=False, out_f32=False, out_n16=True):
    """``bn_apply_nhwc`` for the narrow encoder: ``y`` (the conv result) and ``res`` are fp32 or narrow tensors; the result
    comes back narrow ('n16', what the next conv reads) and/or fp32 ('y'); 'stats' as requested."""
    n, ho, wo, c = y.shape
    lib = _lib.load()
    if dtype is None:
        dtype = y.dtype if y.dtype != torch.float32 else (res.dtype if res is not None else None)
    if dtype is None or dtype == torch.float32:
        raise ValueError("bn_apply_nhwc_n16: pass dtype= when neither y nor res is a narrow tensor")
    r32, r16, _, hr, wr = _bn_apply_args(y, scale, shift, alpha, res, res_scale, res_shift, mask, n16=dtype)
    y32 = y16 = None
    if y.dtype == torch.float32:
        _dev_f32(y, "y")
        y32 = y
    else:
        _dev_n16(y, "y", dtype)
        y16 = y
    out = {}
    if out_f32:
        out["y"] = torch.empty(tuple(y.shape), device=y.device, dtype=torch.float32)
    if out_n16:
        out["n16"] = torch.empty(tuple(y.shape), device=y.device, dtype=dtype)
    if want_stats:
        out["stats"] = _empty((lib.cer_bn_apply_stats_tiles(n * ho * wo), 2, c), scale)
    check(lib.cer_bn_apply_nhwc_n16(ptr(y32), ptr(y16), ptr(scale), ptr(shift), ptr(alpha), ptr(r32), ptr(r16), ptr(res_scale),
                                    ptr(res_shift), ptr(mask), ptr(out.get("y")), ptr(out.get("n16")), ptr(out.get("stats")),
                                    n, ho, wo, c, res_stride, hr, wr, storage_of(dtype), current_stream()),
          "cer_bn_apply_nhwc_n16")
    return out


AUTO_SPLIT_K = os.environ.get("CER_TAIL_SPLITK", "1") != "0"


def auto_split_k(m, cout, kdim):
    """Split-K factor for the small GEMMs of the trainable tail (M = B*L rows): a 1024 x 128 output is 32 tiles of 64 x 64
    on a 256-CU chip, so the K loop is cut until ~256 blocks are in flight (deterministic slabs + one reduce launch)."""
    if not AUTO_SPLIT_K:
        return 1
    tiles = ((m + 63) // 64) * ((cout + 63) // 64)
    if tiles >= 128 or kdim < 256:
        return 1
    return max(1, min(kdim // 128, 256 // tiles, 16))


def linear(x2d, w_packed, bias=None, act=ACT_NONE, split_k=1, residual=None, out=None):
    """[M,K] @ W[Cout,K]^T as a 1x1 conv on an [M,1,1,K] image.  x2d / out may be column
    slices of wider row-major buffers."""
    m, k, x_ld = _rows(x2d, "x2d")
    res = residual.view(m, 1, 1, -1) if residual is not None else None
    y_ld = 0
    if out is not None:
        _, _, y_ld = _rows(out, "out")
        if y_ld == out.shape[1]:
            y_ld = 0
    y = conv2d(x2d, w_packed, 1, 1, bias=bias, act1=act, split_k=split_k, residual=res, out=out,
               x_ld=(0 if x_ld == k else x_ld), y_ld=y_ld, x_shape=(m, 1, 1, k))
    return y if out is not None else y.view(m, -1)


def l2norm_rows(x):
    _dev_f32(x, "x")
    y = torch.empty_like(x)
    check(_lib.load().cer_l2norm_rows(ptr(x), ptr(y), x.shape[0], x.shape[1], current_stream()),
          "cer_l2norm_rows")
    return y


# bench.py sets this to a list to time every matrix-core weight-gradient launch: (Cout, Cin, taps, algorithmic FLOPs, start, end)
WGRAD_TRACE = None


def _wgrad_traced(fn, n, ho, wo, cout, cin, kh, kw):
    if WGRAD_TRACE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    WGRAD_TRACE.append((cout, cin, kh * kw, 2.0 * n * ho * wo * cout * cin * kh * kw, e0, e1))


def conv2d_wgrad(dz, x, kh, kw, stride=1, pad=(0, 0), b3=False):
    """dW [Cout,Cin,KH,KW] (torch layout) from dz [N,Ho,Wo,Cout] and the conv input x [N,H,W,Cin] (both dense NHWC).
    ``b3``: the bf16x3 MFMA kernel with the pixel range split over blocks (Cout, Cin % 4 == 0; other shapes take the
    fp32-MFMA kernel either way).  ``dz`` / ``x`` may be ``Split`` tensors (then both are used split: no conversion in the
    kernel's loader)."""
    split_in = isinstance(dz, Split) or isinstance(x, Split)
    if split_in:
        dz = dz if isinstance(dz, Split) else split_bf16(dz)
        x = x if isinstance(x, Split) else split_bf16(x)
        n, ho, wo, cout = dz.hi.shape
        _, h, w, cin = x.hi.shape
        if cout % 4 or cin % 4:
            raise ValueError("conv2d_wgrad on split tensors needs channel counts that are multiples of 4")
        dw = torch.empty((cout, cin, kh, kw), device=dz.hi.device, dtype=torch.float32)
        lib = _lib.load()
        nbytes = lib.cer_conv2d_wgrad_b3_workspace_bytes(n, ho, wo, cout, cin, kh, kw)
        ws = torch.empty((nbytes // 4,), device=dw.device, dtype=torch.float32) if nbytes else None
        _wgrad_traced(lambda: check(lib.cer_conv2d_wgrad_b3s(ptr(dz.hi), ptr(dz.lo), ptr(x.hi), ptr(x.lo), ptr(dw), n, h, w, ho, wo,
                                                              cout, cin, kh, kw, stride, pad[0], pad[1], ptr(ws), nbytes,
                                                              current_stream()), "cer_conv2d_wgrad_b3s"), n, ho, wo, cout, cin, kh, kw)
        return dw
    _dev_f32(dz, "dz")
    _dev_f32(x, "x")
    n, ho, wo, cout = dz.shape
    _, h, w, cin = x.shape
    dw = _empty((cout, cin, kh, kw), dz)
    if b3 and cout % 4 == 0 and cin % 4 == 0:
        lib = _lib.load()
        nbytes = lib.cer_conv2d_wgrad_b3_workspace_bytes(n, ho, wo, cout, cin, kh, kw)
        ws = _empty((nbytes // 4,), dz) if nbytes else None
        _wgrad_traced(lambda: check(lib.cer_conv2d_wgrad_b3(ptr(dz), ptr(x), ptr(dw), n, h, w, ho, wo, cout, cin, kh, kw, stride,
                                                             pad[0], pad[1], ptr(ws), nbytes, current_stream()),
                                    "cer_conv2d_wgrad_b3"), n, ho, wo, cout, cin, kh, kw)
        return dw
    lib = _lib.load()
    nbytes = lib.cer_conv_wgrad_workspace_bytes(n * ho * wo, cout, cin, kh * kw)
    ws = _empty((nbytes // 4,), dz) if nbytes else None
    check(lib.cer_conv2d_wgrad(ptr(dz), ptr(x), ptr(dw), n, h, w, ho, wo, cout, cin, kh, kw, stride, pad[0], pad[1],
                               ptr(ws), nbytes, current_stream()), "cer_conv2d_wgrad")
    return dw


def prelu_fwd(x, alpha):
    _dev_f32(x, "x")
    _dev_f32(alpha, "alpha", shape=x.shape[-1:])
    y = torch.empty_like(x)
    check(_lib.load().cer_prelu_fwd(ptr(x), ptr(alpha), ptr(y), x.numel() // x.shape[-1], x.shape[-1], current_stream()),
          "cer_prelu_fwd")
    return y


def prelu_split(x, alpha):
    """prelu(x) as a Split tensor in one pass (the conv input a released unit rebuilds from its raw conv result)."""
    _dev_f32(x, "x")
    _dev_f32(alpha, "alpha", shape=x.shape[-1:])
    out = Split.empty(x.shape, x.device)
    c = x.shape[-1]
    check(_lib.load().cer_prelu_split(ptr(x), ptr(alpha), ptr(out.hi), ptr(out.lo), x.numel() // c, c, current_stream()),
          "cer_prelu_split")
    return out


def prelu_bwd(dy, x, alpha, out=None, split_out=False):
    """-> (dx, dalpha): torch's PReLU backward for channels-last tensors.  ``split_out``: dx comes back as a Split tensor (no fp32
    copy is written); ``out``: write dx into this fp32 tensor / Split (a slice of a larger one: chunked calls)."""
    _dev_f32(x, "x")
    _dev_f32(dy, "dy", shape=x.shape)
    _dev_f32(alpha, "alpha", shape=x.shape[-1:])
    terms = torch.empty_like(x)
    c = x.shape[-1]
    if split_out:
        dx = out if out is not None else Split.empty(x.shape, x.device)
        _dev_bf16(dx.hi, "out.hi")
        _dev_bf16(dx.lo, "out.lo")
        check(_lib.load().cer_prelu_bwd_split(ptr(dy), ptr(x), ptr(alpha), None, ptr(dx.hi), ptr(dx.lo), ptr(terms), x.numel() // c, c,
                                              current_stream()), "cer_prelu_bwd_split")
    else:
        dx = out if out is not None else torch.empty_like(x)
        _dev_f32(dx, "out")
        check(_lib.load().cer_prelu_bwd(ptr(dy), ptr(x), ptr(alpha), ptr(dx), ptr(terms), x.numel() // c, c, current_stream()),
              "cer_prelu_bwd")
    return dx, col_sum(terms.view(-1, c))


def l2norm_rows_bwd(dy, x):
    """Gradient of ``l2norm_rows`` w.r.t. its input ``x`` (the un-normalised rows)."""
    _dev_f32(dy, "dy")
    _dev_f32(x, "x")
    dx = torch.empty_like(x)
    check(_lib.load().cer_l2norm_rows_bwd(ptr(dy), ptr(x), ptr(dx), x.shape[0], x.shape[1], current_stream()),
          "cer_l2norm_rows_bwd")
    return dx


def maxpool2x2_nhwc(x):
    _dev_f32(x, "x")
    n, h, w, c = x.shape
    y = _empty((n, h // 2, w // 2, c), x)
    check(_lib.load().cer_maxpool2x2_nhwc(ptr(x), ptr(y), n, h, w, c, current_stream()), "cer_maxpool2x2_nhwc")
    return y


# ------------------------------------------------------------------ train-mode BatchNorm2d (encoder)
def bn_finalize(partials, count, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """[tiles,2,C] partial sums -> (scale, shift) of the batch-statistics BatchNorm; running stats
    are updated in place like torch does in train mode."""
    _dev_f32(partials, "partials")
    if partials.dim() != 3 or partials.shape[1] != 2 or partials.shape[0] == 0 or partials.shape[2] == 0:
        raise ValueError(f"partials: expected a [tiles, 2, C] tensor, got shape {tuple(partials.shape)}")
    tiles, _, c = partials.shape
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _dev_f32(t, n, shape=(c,))
    scale, shift = _empty((c,), partials), _empty((c,), partials)
    lib = _lib.load()
    nbytes = lib.cer_bn_finalize_workspace_bytes(tiles, c)
    ws = torch.empty((nbytes // 8,), device=partials.device, dtype=torch.float64)
    check(lib.cer_bn_finalize(ptr(partials), tiles, c, float(count), ptr(gamma), ptr(beta), ptr(running_mean),
                              ptr(running_var), momentum, eps, ptr(scale), ptr(shift), ptr(ws), nbytes,
                              current_stream()), "cer_bn_finalize")
    return scale, shift


def _dev_f64(t, name, shape):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous float64 tensor on the GPU, got "
                         f"{t.dtype} {t.device} contiguous={t.is_contiguous()}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def bn_partial_sums(partials):
    """[tiles,2,C] partial sums -> [2,C] float64 (sum | sum of squares), reduced exactly as ``bn_finalize`` reduces them.
    The first half of ``bn_finalize`` for synchronised statistics: all-reduce the result, then ``bn_finalize_sums``."""
    _dev_f32(partials, "partials")
    if partials.dim() != 3 or partials.shape[1] != 2 or partials.shape[0] == 0 or partials.shape[2] == 0:
        raise ValueError(f"partials: expected a [tiles, 2, C] tensor, got shape {tuple(partials.shape)}")
    tiles, _, c = partials.shape
    lib = _lib.load()
    nbytes = lib.cer_bn_finalize_workspace_bytes(tiles, c)
    ws = torch.empty((nbytes // 8,), device=partials.device, dtype=torch.float64)
    sums = torch.empty((2, c), device=partials.device, dtype=torch.float64)
    check(lib.cer_bn_partial_sums(ptr(partials), tiles, c, ptr(sums), ptr(ws), nbytes, current_stream()), "cer_bn_partial_sums")
    return sums


def bn_finalize_sums(sums, count, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """``bn_finalize``'s second half: [2,C] float64 sums over ``count`` elements -> (scale, shift); running stats updated in
    place when given.  The same bits as ``bn_finalize`` for the same sums."""
    if sums.dim() != 2 or sums.shape[0] != 2:
        raise ValueError(f"sums: expected a [2, C] tensor, got shape {tuple(sums.shape)}")
    c = sums.shape[1]
    _dev_f64(sums, "sums", (2, c))
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _dev_f32(t, n, shape=(c,))
    if gamma is None or beta is None or (running_mean is None) != (running_var is None):
        raise ValueError("bn_finalize_sums: gamma and beta are required; running_mean and running_var go together")
    if not count > 0:
        raise ValueError(f"bn_finalize_sums: count must be positive, got {count}")
    scale, shift = _empty((c,), gamma), _empty((c,), gamma)
    check(_lib.load().cer_bn_finalize_sums(ptr(sums), c, float(count), ptr(gamma), ptr(beta), ptr(running_mean),
                                           ptr(running_var), momentum, eps, ptr(scale), ptr(shift), current_stream()),
          "cer_bn_finalize_sums")
    return scale, shift


def bn_apply_nhwc(y, scale, shift, alpha=None, res=None, res_stride=1, res_scale=None, res_shift=None, mask=None,
                  want_stats=False):
    """out = mask*prelu(y*scale+shift) + (res*res_scale+res_shift) on NHWC; optionally the partial
    statistics of ``out`` for the next BatchNorm."""
    _dev_f32(y, "y")
    n, ho, wo, c = y.shape
    _, _, _, hr, wr = _bn_apply_args(y, scale, shift, alpha, res, res_scale, res_shift, mask)
    lib = _lib.load()
    out = torch.empty_like(y)
    stats = _empty((lib.cer_bn_apply_stats_tiles(n * ho * wo), 2, c), y) if want_stats else None
    check(lib.cer_bn_apply_nhwc(ptr(y), ptr(scale), ptr(shift), ptr(alpha), ptr(res), ptr(res_scale), ptr(res_shift),
                                ptr(mask), ptr(out), ptr(stats), n, ho, wo, c, res_stride, hr, wr, current_stream()),
          "cer_bn_apply_nhwc")
    return (out, stats) if want_stats else out


def bn_apply_nhwc_b3(y, scale, shift, alpha=None, res=None, res_stride=1, res_scale=None, res_shift=None, mask=None,
                     want_stats=False, out_f32=False, out_split=True):
    """``bn_apply_nhwc`` for the bf16x3 encoder: ``res`` may be a Split tensor, the result comes back as a Split
    (what the next conv reads) and/or fp32.  Returns a dict with 'split', 'y', 'stats' as requested."""
    _dev_f32(y, "y")
    n, ho, wo, c = y.shape
    r_f32, r_hi, r_lo, hr, wr = _bn_apply_args(y, scale, shift, alpha, res, res_scale, res_shift, mask, split=True)
    lib = _lib.load()
    out = {}
    if out_f32:
        out["y"] = torch.empty_like(y)
    if out_split:
        out["split"] = Split.empty(tuple(y.shape), y.device)
    if want_stats:
        out["stats"] = _empty((lib.cer_bn_apply_stats_tiles(n * ho * wo), 2, c), y)
    sp = out.get("split")
    check(lib.cer_bn_apply_nhwc_b3(ptr(y), ptr(scale), ptr(shift), ptr(alpha), ptr(r_f32), ptr(r_hi), ptr(r_lo),
                                   ptr(res_scale), ptr(res_shift), ptr(mask), ptr(out.get("y")),
                                   ptr(sp.hi) if sp is not None else None, ptr(sp.lo) if sp is not None else None,
                                   ptr(out.get("stats")), n, ho, wo, c, res_stride, hr, wr, current_stream()),
          "cer_bn_apply_nhwc_b3")
    return out


def fold_bn_3x3_packed(w_packed, scale, shift, out="f32"):
    """Fold a per-input-channel affine (the BatchNorm in FRONT of a 3x3 / pad 1 / stride 1 conv) into the PACKED weight
    [Cout, Kpad] in one launch: returns (w * scale[cin] in the requested form, bias9 [9, Cout]).  conv(pad0(s*x + t)) =
    conv'(pad0(x)) + sum over the taps INSIDE the image of W_tap . t, which only depends on whether the output pixel sits
    on the first / an inner / the last row and column (9 cases).  ``out``: "f32", "split" (Split) or a narrow torch dtype."""
    _dev_f32(w_packed, "w_packed")
    _dev_f32(scale, "scale")
    _dev_f32(shift, "shift")
    cout, kpad = w_packed.shape
    cin = scale.numel()
    if kpad != conv_kpad(3, 3, cin) or shift.numel() != cin:
        raise ValueError("fold_bn_3x3_packed: w_packed must be the packing of a [Cout, Cin, 3, 3] weight")
    b9 = _empty((9, cout), w_packed)
    wf = hi = lo = None
    storage = STORE_NONE
    if out == "f32":
        res = wf = torch.empty_like(w_packed)
    elif out == "split":
        res = Split.empty((cout, kpad), w_packed.device)
        hi, lo = res.hi, res.lo
    else:
        storage = storage_of(out)
        res = hi = torch.empty((cout, kpad), device=w_packed.device, dtype=out)
    check(_lib.load().cer_fold_bn_3x3(ptr(w_packed), ptr(scale), ptr(shift), cout, cin, ptr(wf), ptr(hi), ptr(lo), storage,
                                      ptr(b9), current_stream()), "cer_fold_bn_3x3")
    return res, b9


def fold_input_bn_3x3(w_oihw, scale, shift):
    """``fold_bn_3x3_packed`` from the torch-layout weight [Cout, Cin, 3, 3]: (packed fp32 weight, bias9)."""
    _dev_f32(w_oihw, "w")
    if w_oihw.shape[2] != 3 or w_oihw.shape[3] != 3:
        raise ValueError("fold_input_bn_3x3: 3x3 kernels only")
    return fold_bn_3x3_packed(pack_conv_weight(w_oihw.contiguous()), scale.contiguous(), shift.contiguous(), "f32")


def gather_rows(src, index):
    """out[i] = src[index[i]] (zeros where index < 0); src [R, C] fp32, index int64 on the same device."""
    _dev_f32(src, "src")
    if index.dtype != torch.int64 or not index.is_cuda or not index.is_contiguous():
        raise ValueError("index: expected a contiguous int64 GPU tensor")
    out = torch.empty((index.numel(), src.shape[1]), device=src.device, dtype=torch.float32)
    check(_lib.load().cer_gather_rows(ptr(src), ptr(index), ptr(out), index.numel(), src.shape[1], src.shape[0],
                                      current_stream()), "cer_gather_rows")
    return out


def sgd_nesterov_flat(param, grad, buf, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True, first_step=False):
    for t, nme in ((param, "param"), (grad, "grad"), (buf, "buf")):
        _dev_f32(t, nme)
    check(_lib.load().cer_sgd_nesterov_flat(ptr(param), ptr(grad), ptr(buf), param.numel(), lr, momentum, dampening,
                                            weight_decay, int(nesterov), int(first_step), current_stream()),
          "cer_sgd_nesterov_flat")


def adam_flat(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              amsgrad=False):
    """torch.optim.Adam's update over flat fp32 buffers in one launch; ``step`` is the count after this update (>= 1)."""
    bufs = [(param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")]
    if amsgrad:
        if max_exp_avg_sq is None:
            raise ValueError("max_exp_avg_sq: required with amsgrad")
        bufs.append((max_exp_avg_sq, "max_exp_avg_sq"))
    for t, nme in bufs:
        _dev_f32(t, nme)
        if t.numel() != param.numel():
            raise ValueError(f"{nme}: expected {param.numel()} elements, got {t.numel()}")
    check(_lib.load().cer_adam_flat(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq),
                                    ptr(max_exp_avg_sq) if amsgrad else None, param.numel(), float(lr), float(betas[0]),
                                    float(betas[1]), float(eps), float(weight_decay), int(amsgrad), int(step),
                                    current_stream()), "cer_adam_flat")


def _dev_scalar(t, name, dtype, device):
    """A one-element tensor of ``dtype`` on ``device`` (GradScaler's scale / found_inf, the applied-step counter)."""
    if not (t.is_cuda and t.dtype == dtype and t.numel() == 1 and t.device == device and t.is_contiguous()):
        raise ValueError(f"{name}: expected a one-element {dtype} tensor on {device}, got {t.dtype} {t.device} numel={t.numel()}")


def amp_check_unscale_flat(grad, found_inf, inv_scale=None):
    """``torch._amp_foreach_non_finite_check_and_unscale_`` over the flat fp32 gradient bucket in one launch: ``found_inf``
    (fp32 device scalar) becomes 1 if any element is Inf / NaN; with ``inv_scale`` (fp32 device scalar) the bucket is unscaled
    in place, without it only checked."""
    _dev_f32(grad, "grad")
    _dev_scalar(found_inf, "found_inf", torch.float32, grad.device)
    if inv_scale is not None:
        _dev_scalar(inv_scale, "inv_scale", torch.float32, grad.device)
    check(_lib.load().cer_amp_check_unscale_flat(ptr(grad), grad.numel(), ptr(inv_scale), ptr(found_inf), current_stream()),
          "cer_amp_check_unscale_flat")


def _amp_scalars(grad, grad_scale, found_inf, applied):
    if grad_scale is not None:
        _dev_scalar(grad_scale, "grad_scale", torch.float32, grad.device)
    _dev_scalar(found_inf, "found_inf", torch.float32, grad.device)
    _dev_scalar(applied, "applied", torch.int64, grad.device)


def sgd_nesterov_flat_amp(param, grad, buf, lr, grad_scale, found_inf, applied, momentum=0.9, dampening=0.0, weight_decay=0.0,
                          nesterov=True):
    """``sgd_nesterov_flat`` under a GradScaler: skipped on the device when ``found_inf`` != 0, gradients unscaled in place by
    ``grad_scale`` (None: already unscaled), ``applied`` (int64 device scalar) counts the applied steps and decides the first
    step."""
    for t, nme in ((param, "param"), (grad, "grad"), (buf, "buf")):
        _dev_f32(t, nme)
        if t.numel() != param.numel():
            raise ValueError(f"{nme}: expected {param.numel()} elements, got {t.numel()}")
    _amp_scalars(grad, grad_scale, found_inf, applied)
    check(_lib.load().cer_sgd_nesterov_flat_amp(ptr(param), ptr(grad), ptr(buf), param.numel(), lr, momentum, dampening,
                                                weight_decay, int(nesterov), ptr(grad_scale), ptr(found_inf), ptr(applied),
                                                current_stream()), "cer_sgd_nesterov_flat_amp")


def adam_flat_amp(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, bias_correction, grad_scale, found_inf, applied,
                  betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
    """``adam_flat`` under a GradScaler: as ``sgd_nesterov_flat_amp``; the step is ``applied + 1`` on the device and its bias
    corrections come from ``bias_correction`` [T, 2] float64 (1 - b1^k, sqrt(1 - b2^k) for k = 1..T)."""
    bufs = [(param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")]
    if amsgrad:
        if max_exp_avg_sq is None:
            raise ValueError("max_exp_avg_sq: required with amsgrad")
        bufs.append((max_exp_avg_sq, "max_exp_avg_sq"))
    for t, nme in bufs:
        _dev_f32(t, nme)
        if t.numel() != param.numel():
            raise ValueError(f"{nme}: expected {param.numel()} elements, got {t.numel()}")
    if not (bias_correction.is_cuda and bias_correction.dtype == torch.float64 and bias_correction.is_contiguous()
            and bias_correction.dim() == 2 and bias_correction.shape[1] == 2 and bias_correction.shape[0] >= 1
            and bias_correction.device == param.device):
        raise ValueError("bias_correction: expected a contiguous [T >= 1, 2] float64 tensor on the parameters' device")
    _amp_scalars(grad, grad_scale, found_inf, applied)
    check(_lib.load().cer_adam_flat_amp(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq),
                                        ptr(max_exp_avg_sq) if amsgrad else None, param.numel(), float(lr), float(betas[0]),
                                        float(betas[1]), float(eps), float(weight_decay), int(amsgrad), ptr(bias_correction),
                                        bias_correction.shape[0], ptr(grad_scale), ptr(found_inf), ptr(applied),
                                        current_stream()), "cer_adam_flat_amp")


# ------------------------------------------------------------------ trainable tail
def weight_norm_fwd(v, g):
    """v [Cout,Cin,k], g [Cout,1,1] -> (w [Cout,Cin,k], norm [Cout])."""
    _dev_f32(v, "v")
    _dev_f32(g, "g")
    rows, e = v.shape[0], v.numel() // v.shape[0]
    w, norm = torch.empty_like(v), _empty((rows,), v)
    check(_lib.load().cer_weight_norm_fwd(ptr(v), ptr(g), ptr(w), ptr(norm), rows, e, current_stream()),
          "cer_weight_norm_fwd")
    return w, norm


def weight_norm_fwd_packed(v, g):
    """``weight_norm_fwd`` of a [Cout,Cin,k] filter plus, from the same launch, the packed forward weight [Cout,Kpad(k,1,Cin)] and
    the flipped / transposed data-gradient weight [Cin,Kpad(k,1,Cout)] (``pack_conv_weight`` twice): (w, norm, wp, wt)."""
    _dev_f32(v, "v")
    _dev_f32(g, "g")
    cout, cin, k = v.shape
    w, norm = torch.empty_like(v), _empty((cout,), v)
    wp, wt = _empty((cout, conv_kpad(k, 1, cin)), v), _empty((cin, conv_kpad(k, 1, cout)), v)
    check(_lib.load().cer_weight_norm_fwd_packed(ptr(v), ptr(g), ptr(w), ptr(norm), ptr(wp), ptr(wt), cout, cin, k, current_stream()),
          "cer_weight_norm_fwd_packed")
    return w, norm, wp, wt


def conv1d_wgrad_weight_norm_bwd(dz, x, seq_len, k, dil, v, g, norm):
    """(dv, dg) of a weight-normed causal conv from dz [R,Cout] and the layer input x [R,Cin]: ``conv1d_wgrad`` +
    ``weight_norm_bwd`` with the split-R partial sums folded inside the second kernel (two launches)."""
    r, cout, dz_ld = _rows(dz, "dz")
    r2, cin, x_ld = _rows(x, "x")
    if r != r2:
        raise ValueError("dz and x must have the same number of rows")
    for t, n in ((v, "v"), (g, "g"), (norm, "norm")):
        _dev_f32(t, n)
    lib = _lib.load()
    nbytes = max(lib.cer_conv_wgrad_workspace_bytes(r, cout, cin, k), cout * cin * k * 4)
    ws = _empty((nbytes // 4,), dz)
    dv, dg = torch.empty_like(v), torch.empty_like(g)       # (dg in g's [Cout,1,1] shape, as weight_norm_bwd returns it)
    check(lib.cer_conv1d_wgrad_weight_norm_bwd(ptr(dz), dz_ld, ptr(x), x_ld, r, seq_len, cout, cin, k, dil, ptr(v), ptr(g), ptr(norm),
                                               ptr(dv), ptr(dg), ptr(ws), nbytes, current_stream()), "cer_conv1d_wgrad_weight_norm_bwd")
    return dv, dg


def weight_norm_bwd(dw, v, g, norm):
    for t, n in ((dw, "dw"), (v, "v"), (g, "g"), (norm, "norm")):
        _dev_f32(t, n)
    rows, e = v.shape[0], v.numel() // v.shape[0]
    dv, dg = torch.empty_like(v), torch.empty_like(g)
    check(_lib.load().cer_weight_norm_bwd(ptr(dw), ptr(v), ptr(g), ptr(norm), ptr(dv), ptr(dg), rows, e,
                                          current_stream()), "cer_weight_norm_bwd")
    return dv, dg


def conv1d_wgrad(dz, x, seq_len, k, dil):
    """dW [Cout,Cin,k] from dz [R,Cout] and the layer input x [R,Cin] (both may be column slices, at any offset and pitch:
    an operand whose rows do not start on 16-byte boundaries is read with scalar loads)."""
    r, cout, dz_ld = _rows(dz, "dz")
    r2, cin, x_ld = _rows(x, "x")
    if r != r2:
        raise ValueError("dz and x must have the same number of rows")
    dw = _empty((cout, cin, k), dz)
    lib = _lib.load()
    nbytes = lib.cer_conv_wgrad_workspace_bytes(r, cout, cin, k)
    ws = _empty((nbytes // 4,), dz) if nbytes else None
    check(lib.cer_conv1d_wgrad(ptr(dz), dz_ld, ptr(x), x_ld, ptr(dw), r, seq_len, cout, cin, k, dil, ptr(ws), nbytes,
                               current_stream()), "cer_conv1d_wgrad")
    return dw


def _col_ws(r, c, like):
    nbytes = _lib.load().cer_col_sum_workspace_bytes(r, c)
    return (_empty((nbytes // 4,), like) if nbytes else None), nbytes


def col_sum(a):
    """Column sums of a [R,C] tensor (bias gradients)."""
    r, c, ld = _rows(a, "a")
    out = _empty((c,), a)
    ws, nbytes = _col_ws(r, c, a)
    check(_lib.load().cer_col_sum(ptr(a), ld, None, 0, None, None, ptr(out), r, c, ptr(ws), nbytes,
                                  current_stream()), "cer_col_sum")
    return out


def act_mask_bwd(dy, y, mask=None, slope=LEAKY_SLOPE):
    _dev_f32(dy, "dy")
    for t, n in ((y, "y"), (mask, "mask")):
        _dev_f32(t, n, shape=dy.shape)
    dz = torch.empty_like(dy)
    check(_lib.load().cer_act_mask_bwd(ptr(dy), ptr(y), ptr(mask), ptr(dz), dy.numel(), slope, current_stream()),
          "cer_act_mask_bwd")
    return dz


def fc_bwd(da, act=None, out_split=True, out_f32=False):
    """The elementwise part of a fully-connected layer's backward in ONE pass: dz = da * (act > 0) (``act`` = the layer's
    saved post-ReLU output [R, C] -- fp32, ``Split`` or one bf16 / fp16 plane; None: no mask, the output layer), stored as a
    ``Split`` ('split') and / or fp32 ('f32'), and the bias gradient 'db' = column sums of dz (fixed order, bit-identical
    from run to run).  ``da`` may be a column slice of a wider row-major buffer.  Returns a dict."""
    if not (da.is_cuda and da.dtype == torch.float32 and da.dim() == 2 and da.stride(1) == 1):
        raise ValueError("da: expected a 2-D float32 GPU tensor with unit column stride")
    r, c = da.shape
    ld = da.stride(0) if r > 1 else c
    if c % 4:
        raise ValueError(f"fc_bwd: C = {c} is not a multiple of 4")
    if not (out_split or out_f32):
        raise ValueError("fc_bwd: ask for the split planes, the fp32 dz, or both")
    a = a_lo = None
    kind = _lib.FC_ACT_NONE
    if isinstance(act, Split):
        _dev_bf16(act.hi, "act.hi")
        _dev_bf16(act.lo, "act.lo")
        a, a_lo, kind = act.hi, act.lo, _lib.FC_ACT_SPLIT
    elif act is not None:
        if act.dtype == torch.float32:
            _dev_f32(act, "act")
            kind = _lib.FC_ACT_F32
        else:
            _dev_n16(act, "act")
            kind = _lib.FC_ACT_BF16 if act.dtype == torch.bfloat16 else _lib.FC_ACT_F16
        a = act
    if a is not None and a.numel() != r * c:
        raise ValueError(f"act: expected {r * c} elements (the shape of da), got {tuple(a.shape)}")
    res = {"db": torch.empty((c,), device=da.device, dtype=torch.float32)}
    if out_split:
        res["split"] = Split.empty((r, c), da.device)
    if out_f32:
        res["f32"] = torch.empty((r, c), device=da.device, dtype=torch.float32)
    lib = _lib.load()
    nbytes = lib.cer_fc_bwd_workspace_bytes(r, c)
    ws = torch.empty((nbytes // 4,), device=da.device, dtype=torch.float32) if nbytes else None
    sp = res.get("split")
    check(lib.cer_fc_bwd_elem(ptr(da), ld, ptr(a), ptr(a_lo), kind, ptr(sp.hi) if sp is not None else None,
                              ptr(sp.lo) if sp is not None else None, ptr(res.get("f32")), ptr(res["db"]), r, c, ptr(ws), nbytes,
                              current_stream()), "cer_fc_bwd_elem")
    return res


def tblock_tail_bwd(dout, out, a2, mask2=None, slope=LEAKY_SLOPE):
    _dev_f32(dout, "dout")
    for t, n in ((out, "out"), (a2, "a2"), (mask2, "mask2")):
        _dev_f32(t, n, shape=dout.shape)
    du, dz2 = torch.empty_like(dout), torch.empty_like(dout)
    check(_lib.load().cer_tblock_tail_bwd(ptr(dout), ptr(out), ptr(a2), ptr(mask2), ptr(du), ptr(dz2),
                                          dout.numel(), slope, current_stream()), "cer_tblock_tail_bwd")
    return du, dz2


def bn_rows_fwd(x, w, b, running_mean, running_var, train, eps=1e-5, momentum=0.1, out=None):
    """BatchNorm over the rows of x [R,C].  Returns (y, save_mean, save_invstd); the saves are
    None in eval mode.  Running stats are updated in place when ``train``."""
    r, c, x_ld = _rows(x, "x")
    for t, n in ((w, "w"), (b, "b"), (running_mean, "running_mean"), (running_var, "running_var")):
        _dev_f32(t, n, shape=(c,))
    if out is None:
        out = _empty((r, c), x)
    _, _, y_ld = _rows(out, "out")
    _dev_f32(out, "out", contiguous=False, shape=(r, c))
    sm = _empty((c,), x) if train else None
    si = _empty((c,), x) if train else None
    lib = _lib.load()
    nbytes = lib.cer_bn_rows_fwd_workspace_bytes(r, c) if train else 0
    ws = _empty((nbytes // 4,), x) if nbytes else None
    check(lib.cer_bn_rows_fwd(ptr(x), x_ld, ptr(w), ptr(b), ptr(running_mean), ptr(running_var), ptr(sm),
                              ptr(si), ptr(out), y_ld, r, c, 1 if train else 0, eps, momentum, ptr(ws), nbytes,
                              current_stream()), "cer_bn_rows_fwd")
    return out, sm, si


def bn_rows_stats(x, running_mean, running_var, eps=1e-5, momentum=0.1):
    """Train-mode statistics of the rows of x [R,C] alone: (save_mean, save_invstd), running buffers updated in place like
    ``bn_rows_fwd(train=True)``; no output tensor is written."""
    r, c, x_ld = _rows(x, "x")
    _dev_f32(running_mean, "running_mean", shape=(c,))
    _dev_f32(running_var, "running_var", shape=(c,))
    sm, si = _empty((c,), x), _empty((c,), x)
    lib = _lib.load()
    nbytes = lib.cer_bn_rows_fwd_workspace_bytes(r, c)
    ws = _empty((nbytes // 4,), x) if nbytes else None
    check(lib.cer_bn_rows_fwd(ptr(x), x_ld, None, None, ptr(running_mean), ptr(running_var), ptr(sm), ptr(si), None, 0, r, c, 1,
                              eps, momentum, ptr(ws), nbytes, current_stream()), "cer_bn_rows_fwd")
    return sm, si


def bn_rows_bwd(dy, x, save_mean, save_invstd, w, train=True, split_out=False, add=None):
    """(dx, dw, db) of the row BatchNorm over x [R,C] (dense or a column slice): ``bn_rows_bwd_sums``, then
    ``bn_rows_bwd_apply`` with those sums over R rows.  ``split_out`` (train mode, dense rows): dx as a Split tensor written by
    the apply pass itself.  ``add`` (train mode, dense rows): dx = BatchNorm-backward(dy) + add in the same pass."""
    return _bn_rows_bwd(dy, x, save_mean, save_invstd, w, train, split_out, add, None)


def _bn_rows_bwd(dy, x, save_mean, save_invstd, w, train, split_out, add, global_sums):
    """``bn_rows_bwd`` with the operands checked once; in train mode ``global_sums`` (None: the identity) maps the local
    [2,C] sums and R to the sums and row count that dx is taken over (a synchronised BatchNorm's exchange)."""
    r, c, dy_ld, x_ld = _bn_rows_bwd_check("bn_rows_bwd", dy, x, (save_mean, save_invstd, w), train, split_out, add)
    sums = _bn_rows_bwd_sums(dy, dy_ld, x, x_ld, save_mean, save_invstd, r, c)
    total, count = global_sums(sums, r) if train and global_sums is not None else (sums, r)
    dx = _bn_rows_bwd_apply(dy, dy_ld, x, x_ld, save_mean, save_invstd, w, total, count, train, split_out, add, r, c)
    return dx, sums[1], sums[0]


# ------------------------------------------------------------------ row BatchNorm split at its statistics (synchronised BN)
def bn_rows_moments(x):
    """(count, mean, M2) per channel of the rows of x [R,C] (dense or a column slice) as [3,C] float64 -- what a rank
    contributes to synchronised statistics (see cer_bn_rows_merge for why these and not raw sums)."""
    r, c, x_ld = _rows(x, "x")
    if r == 0 or c == 0:
        raise ValueError(f"x: expected a non-empty [R, C] tensor, got shape {tuple(x.shape)}")
    moments = torch.empty((3, c), device=x.device, dtype=torch.float64)
    check(_lib.load().cer_bn_rows_moments(ptr(x), x_ld, r, c, ptr(moments), current_stream()), "cer_bn_rows_moments")
    return moments


def bn_rows_merge(moments, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """[K,3,C] moment blocks (K ranks, in rank order) -> (save_mean, save_invstd) of their union; the running buffers, when
    given, take the union's mean and unbiased variance in place."""
    if moments.dim() != 3 or moments.shape[1] != 3 or moments.shape[0] == 0 or moments.shape[2] == 0:
        raise ValueError(f"moments: expected a [K, 3, C] tensor, got shape {tuple(moments.shape)}")
    k, _, c = moments.shape
    _dev_f64(moments, "moments", (k, 3, c))
    _dev_f32(running_mean, "running_mean", shape=(c,))
    _dev_f32(running_var, "running_var", shape=(c,))
    if (running_mean is None) != (running_var is None):
        raise ValueError("bn_rows_merge: running_mean and running_var go together")
    sm = torch.empty((c,), device=moments.device, dtype=torch.float32)
    si = torch.empty((c,), device=moments.device, dtype=torch.float32)
    check(_lib.load().cer_bn_rows_merge(ptr(moments), k, c, eps, momentum, ptr(sm), ptr(si), ptr(running_mean),
                                        ptr(running_var), current_stream()), "cer_bn_rows_merge")
    return sm, si


def bn_rows_apply(x, mean, invstd, w, b, out=None):
    """y = (x - mean) * invstd * w + b over the rows of x [R,C]; ``out`` may be a column slice of a wider buffer."""
    r, c, x_ld = _rows(x, "x")
    for t, n in ((mean, "mean"), (invstd, "invstd"), (w, "w"), (b, "b")):
        if t is None:
            raise ValueError(f"bn_rows_apply: {n} is required")
        _dev_f32(t, n, shape=(c,))
    if out is None:
        out = _empty((r, c), x)
    _, _, y_ld = _rows(out, "out")
    _dev_f32(out, "out", contiguous=False, shape=(r, c))
    check(_lib.load().cer_bn_rows_apply(ptr(x), x_ld, ptr(mean), ptr(invstd), ptr(w), ptr(b), ptr(out), y_ld, r, c,
                                        current_stream()), "cer_bn_rows_apply")
    return out


def _bn_rows_bwd_check(fn, dy, x, vecs, train=True, split_out=False, add=None):
    """The operands of the row BatchNorm backward, refused before any launch; ``vecs``: (save_mean, save_invstd[, w]), the
    [C] vectors the call reads.  Returns (R, C, dy pitch, x pitch)."""
    r, c, dy_ld = _rows(dy, "dy")
    _, _, x_ld = _rows(x, "x")
    _dev_f32(x, "x", contiguous=False, shape=(r, c))
    for t, n in zip(vecs, ("save_mean", "save_invstd", "w")):
        if t is None:
            raise ValueError(f"{fn}: {n} is required")
        _dev_f32(t, n, shape=(c,))
    if split_out or add is not None:   # the released encoder units' float4 passes
        if not train or (split_out and add is not None):
            raise ValueError(f"{fn}: split_out / add are train mode, and add needs the fp32 result (split_out=False)")
        _dense_rows4(dy, "dy")
        _dense_rows4(x, "x")
        if add is not None:
            _dense_rows4(add, "add")
            _dev_f32(add, "add", shape=(r, c))
    return r, c, dy_ld, x_ld


def _bn_rows_bwd_sums(dy, dy_ld, x, x_ld, save_mean, save_invstd, r, c):
    sums = _empty((2, c), x)
    ws, nbytes = _col_ws(r, c, x)
    check(_lib.load().cer_bn_rows_bwd_sums(ptr(dy), dy_ld, ptr(x), x_ld, ptr(save_mean), ptr(save_invstd), ptr(sums), r, c,
                                           ptr(ws), nbytes, current_stream()), "cer_bn_rows_bwd_sums")
    return sums


def _bn_rows_bwd_apply(dy, dy_ld, x, x_ld, save_mean, save_invstd, w, sums, count, train, split_out, add, r, c):
    dx = Split.empty((r, c), x.device) if split_out else _empty((r, c), x)
    f32, hi, lo = (None, dx.hi, dx.lo) if split_out else (dx, None, None)
    check(_lib.load().cer_bn_rows_bwd_apply(ptr(dy), dy_ld, ptr(x), x_ld, ptr(save_mean), ptr(save_invstd), ptr(w), ptr(sums),
                                            float(count), 1 if train else 0, ptr(add), ptr(f32), ptr(hi), ptr(lo), r, c,
                                            current_stream()), "cer_bn_rows_bwd_apply")
    return dx


def bn_rows_bwd_sums(dy, x, save_mean, save_invstd):
    """[2,C] float32 = (sum dy, sum dy * x_hat) over the local rows: this rank's db and dw, and its contribution to the
    global sums of a synchronised backward."""
    r, c, dy_ld, x_ld = _bn_rows_bwd_check("bn_rows_bwd_sums", dy, x, (save_mean, save_invstd))
    return _bn_rows_bwd_sums(dy, dy_ld, x, x_ld, save_mean, save_invstd, r, c)


def bn_rows_bwd_apply(dy, x, save_mean, save_invstd, w, sums, count, *, train=True, split_out=False, add=None):
    """dx of the row BatchNorm over the local rows from GIVEN [2,C] sums (sum dy | sum dy * x_hat) over ``count`` rows (the
    global batch's under synchronised BatchNorm; eval mode reads neither).  ``split_out`` / ``add`` as in ``bn_rows_bwd``."""
    r, c, dy_ld, x_ld = _bn_rows_bwd_check("bn_rows_bwd_apply", dy, x, (save_mean, save_invstd, w), train, split_out,
                                        add)
    if sums is None:
        raise ValueError("bn_rows_bwd_apply: sums is required")
    _dev_f32(sums, "sums", shape=(2, c))
    if not count > 0:
        raise ValueError(f"bn_rows_bwd_apply: count must be positive, got {count}")
    return _bn_rows_bwd_apply(dy, dy_ld, x, x_ld, save_mean, save_invstd, w, sums, count, train, split_out, add, r, c)


def _dense_rows4(t, name):
    """A contiguous [R,C] float32 GPU tensor with C % 4 == 0 and a 16-byte-aligned base (the float4 row passes).  Returns (R, C)."""
    r, c = _dense2d(t, name)
    if r == 0 or c == 0 or c % 4 or t.data_ptr() % 16:
        raise ValueError(f"{name}: expected non-empty dense rows with C % 4 == 0 and a 16-byte-aligned base, got shape "
                         f"{tuple(t.shape)}")
    return r, c


def bn_rows_moments_large(x):
    """``bn_rows_moments`` for the released encoder units' large row counts: [3,C] float64 (count, mean, M2) of the dense rows
    of x [R,C] (C % 4 == 0) from one read of x by many row slabs, merged in float64 in a fixed order."""
    r, c = _dense_rows4(x, "x")
    lib = _lib.load()
    nbytes = lib.cer_bn_rows_moments_large_workspace_bytes(r, c)
    ws = _empty((nbytes // 4,), x)
    moments = torch.empty((3, c), device=x.device, dtype=torch.float64)
    check(lib.cer_bn_rows_moments_large(ptr(x), r, c, ptr(moments), ptr(ws), nbytes, current_stream()),
          "cer_bn_rows_moments_large")
    return moments


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _check_qkv(qkv_list, num_heads, head_dim):
    """Every modality's qkv a contiguous [R, H*3*hd] tensor with the same R.  Returns (R, M).  The head dim and the
    modality count (1..4) are the C dispatcher's to refuse."""
    if len(qkv_list) == 0:
        raise ValueError("qkv_list: expected at least one modality")
    r = qkv_list[0].shape[0] if qkv_list[0].dim() == 2 else -1
    for i, t in enumerate(qkv_list):
        _dev_f32(t, f"qkv[{i}]", shape=(r, num_heads * 3 * head_dim))
    return r, len(qkv_list)


def lfan_attn_fwd(qkv_list, num_heads, head_dim):
    """qkv_list: per modality [R, H*3*hd] -> (vals [R, H*M*hd], probs [R,H,M,M])."""
    r, m = _check_qkv(qkv_list, num_heads, head_dim)
    vals = _empty((r, num_heads * m * head_dim), qkv_list[0])
    probs = _empty((r, num_heads, m, m), qkv_list[0])
    check(_lib.load().cer_lfan_attn_fwd(_ptr_array(qkv_list), ptr(vals), ptr(probs), r, num_heads, m, head_dim,
                                        current_stream()), "cer_lfan_attn_fwd")
    return vals, probs


def lfan_attn_bwd(qkv_list, dvals, probs, num_heads, head_dim):
    r, m = _check_qkv(qkv_list, num_heads, head_dim)
    _dev_f32(dvals, "dvals", shape=(r, num_heads * m * head_dim))
    _dev_f32(probs, "probs", shape=(r, num_heads, m, m))
    dqkv = [torch.empty_like(t) for t in qkv_list]
    check(_lib.load().cer_lfan_attn_bwd(_ptr_array(qkv_list), ptr(dvals), ptr(probs), _ptr_array(dqkv), r,
                                        num_heads, m, head_dim, current_stream()), "cer_lfan_attn_bwd")
    return dqkv


def layernorm_fwd(x, gamma, beta, mask=None, eps=1e-5, out=None, save=True):
    """y = LN(x * mask) * gamma + beta over the rows of a dense x [R,C]; ``out`` may be a column slice of a wider buffer."""
    r, c = _dense2d(x, "x")
    _dev_f32(mask, "mask", shape=(r, c))
    _dev_f32(gamma, "gamma", shape=(c,))
    _dev_f32(beta, "beta", shape=(c,))
    if out is None:
        out = _empty((r, c), x)
    _, _, y_ld = _rows(out, "out")
    _dev_f32(out, "out", contiguous=False, shape=(r, c))
    mean = _empty((r,), x) if save else None
    rstd = _empty((r,), x) if save else None
    check(_lib.load().cer_layernorm_fwd(ptr(x), ptr(mask), ptr(gamma), ptr(beta), ptr(out), y_ld, ptr(mean),
                                        ptr(rstd), r, c, eps, current_stream()), "cer_layernorm_fwd")
    return out, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, mask=None):
    """dy may be a column slice of a wider buffer; x and mask are read at pitch C, so they must be dense."""
    r, c, dy_ld = _rows(dy, "dy")
    _dev_f32(x, "x", shape=(r, c))
    _dev_f32(mask, "mask", shape=(r, c))
    _dev_f32(gamma, "gamma", shape=(c,))
    _dev_f32(mean, "mean", shape=(r,))
    _dev_f32(rstd, "rstd", shape=(r,))
    dx, scratch = _empty((r, c), x), _empty((r, c), x)
    dg, db = _empty((c,), x), _empty((c,), x)
    ws, nbytes = _col_ws(r, c, x)
    check(_lib.load().cer_layernorm_bwd(ptr(dy), dy_ld, ptr(x), ptr(mask), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx),
                                        ptr(dg), ptr(db), ptr(scratch), r, c, ptr(ws), nbytes, current_stream()),
          "cer_layernorm_bwd")
    return dx, dg, db


class _LabelCheck:
    """Deferred check of the kernel's bad-label counter: the count travels to pinned host memory asynchronously and is
    looked at on the NEXT call (or by ``flush()``), so validating the labels costs no device synchronisation per step."""
    pending = []

    @classmethod
    def push(cls, count_dev):
        host = torch.empty((1,), dtype=torch.int32, pin_memory=True)
        host.copy_(count_dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        cls.pending.append((host, ev))

    @classmethod
    def poll(cls, wait=False):
        keep = []
        for host, ev in cls.pending:
            if wait:
                ev.synchronize()
            if ev.query():
                if int(host[0]) != 0:
                    cls.pending = []
                    raise IndexError(f"cross_entropy: {int(host[0])} target(s) out of bounds (valid: 0 .. n_classes-1, or "
                                     "-100 = ignore_index), as nn.CrossEntropyLoss raises; the step's loss is NaN")
            else:
                keep.append((host, ev))
        cls.pending = keep


def flush_label_check():
    """Wait for the outstanding label checks (call before trusting a finished epoch; tests call it)."""
    _LabelCheck.poll(wait=True)


def cross_entropy(logits2d, labels_f32, want_grad=True, check_labels=True):
    """Mean CE over rows; labels are float32 class ids (cast like ``.long()``), -100 = ignore_index.  Returns
    (loss scalar tensor, dlogits or None).  Out-of-range labels raise IndexError -- from this call when the counter of an
    earlier call has arrived, at the latest from ``flush_label_check()``; the affected step's loss is NaN either way."""
    r, c = _dense2d(logits2d, "logits")
    _dev_f32(labels_f32, "labels")
    if labels_f32.numel() != r:
        raise ValueError(f"cross_entropy: {labels_f32.numel()} labels for {r} rows")
    loss = _empty((), logits2d)
    dl = torch.empty_like(logits2d) if want_grad else None
    bad = torch.empty((1,), device=logits2d.device, dtype=torch.int32) if check_labels else None
    if check_labels:
        _LabelCheck.poll()
    check(_lib.load().cer_cross_entropy(ptr(logits2d), ptr(labels_f32), ptr(loss), ptr(dl), ptr(bad), r, c, current_stream()),
          "cer_cross_entropy")
    if check_labels:
        _LabelCheck.push(bad)
    return loss, dl


def dropout_mask(shape, p, seed, offset, device):
    if torch.device(device).type != "cuda":   # the kernel would write through a host pointer
        raise ValueError(f"dropout_mask: expected a GPU device, got {device}")
    m = torch.empty(shape, device=device, dtype=torch.float32)
    check(_lib.load().cer_dropout_mask(ptr(m), m.numel(), p, seed, offset, current_stream()), "cer_dropout_mask")
    return m


def leaky_relu(x, slope=LEAKY_SLOPE):
    _dev_f32(x, "x")
    y = torch.empty_like(x)
    check(_lib.load().cer_leaky_relu_fwd(ptr(x), ptr(y), x.numel(), slope, current_stream()), "cer_leaky_relu_fwd")
    return y


def tanh_fwd(x):
    """y = tanh(x) (evaluated in double, rounded once); any shape."""
    _dev_f32(x, "x")
    if x.numel() == 0:
        raise ValueError("tanh_fwd: empty tensor")
    y = torch.empty_like(x)
    check(_lib.load().cer_tanh_fwd(ptr(x), ptr(y), x.numel(), current_stream()), "cer_tanh_fwd")
    return y


def tanh_bwd(dy, y):
    """dx = dy * (1 - y^2) from the saved output ``y`` of ``tanh_fwd``."""
    _dev_f32(y, "y")
    _dev_f32(dy, "dy", shape=y.shape)
    if y.numel() == 0:
        raise ValueError("tanh_bwd: empty tensor")
    dx = torch.empty_like(y)
    check(_lib.load().cer_tanh_bwd(ptr(dy), ptr(y), ptr(dx), y.numel(), current_stream()), "cer_tanh_bwd")
    return dx


def ccc_loss(gold, pred, want_grad=True):
    """The reference's ``CCCLoss()(gold, pred)`` (base/loss_function.py) on [B, L, D] float32 tensors: (loss scalar tensor,
    d loss / d pred or None).  Double arithmetic, no atomics: two calls give identical bits."""
    _dev_f32(gold, "gold")
    _dev_f32(pred, "pred", shape=gold.shape)
    if gold.dim() != 3 or gold.numel() == 0:
        raise ValueError(f"ccc_loss: expected non-empty [B, L, D] tensors, got shape {tuple(gold.shape)}")
    b, l, d = gold.shape
    loss = _empty((), pred)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = torch.empty((b * d,), device=pred.device, dtype=torch.float64)
    check(_lib.load().cer_ccc_loss(ptr(gold), ptr(pred), ptr(loss), ptr(dpred), ptr(ws), b, l, d, current_stream()),
          "cer_ccc_loss")
    return loss, dpred


def regression_moments(pred, label, video_offsets):
    """pred, label [R] float32 (the frames of V videos, concatenated); ``video_offsets``: V+1 host integers rising strictly
    from 0 to R (the kernel reads the rows unchecked, so anything else is refused here) -> [V, 8] float64
    ``{n, mean_p, mean_l, M2_p, M2_l, C_pl, SSE, 0}``."""
    _dev_f32(pred, "pred")
    _dev_f32(label, "label", shape=pred.shape)
    if pred.dim() != 1 or not 0 < pred.numel() < 2 ** 31:
        raise ValueError(f"regression_moments: expected non-empty [R] tensors (R < 2^31), got shape {tuple(pred.shape)}")
    off = [int(o) for o in video_offsets]
    r = pred.numel()
    if len(off) < 2 or off[0] != 0 or off[-1] != r or any(b <= a for a, b in zip(off, off[1:])):
        raise ValueError(f"regression_moments: video_offsets must rise strictly from 0 to {r}, got {off}")
    v = len(off) - 1
    off_d = torch.tensor(off, dtype=torch.int32, device=pred.device)
    out = torch.empty((v, 8), device=pred.device, dtype=torch.float64)
    check(_lib.load().cer_regression_moments(ptr(pred), ptr(label), ptr(off_d), v, r, ptr(out), current_stream()),
          "cer_regression_moments")
    return out


def softmax_gate_fwd(z, c):
    _dense2d(z, "z")
    _dev_f32(c, "c", shape=z.shape)
    out, prob = torch.empty_like(z), torch.empty_like(z)
    check(_lib.load().cer_softmax_gate_fwd(ptr(z), ptr(c), ptr(out), ptr(prob), z.shape[0], z.shape[1], current_stream()),
          "cer_softmax_gate_fwd")
    return out, prob


def softmax_gate_bwd(dout, prob, c):
    _dense2d(dout, "dout")
    for t, n in ((prob, "prob"), (c, "c")):
        _dev_f32(t, n, shape=dout.shape)
    dz, dc = torch.empty_like(dout), torch.empty_like(dout)
    check(_lib.load().cer_softmax_gate_bwd(ptr(dout), ptr(prob), ptr(c), ptr(dz), ptr(dc), dout.shape[0], dout.shape[1],
                                           current_stream()), "cer_softmax_gate_bwd")
    return dz, dc


def copy_cols(x, out):
    r, c, x_ld = _rows(x, "x")
    _, _, y_ld = _rows(out, "out")
    _dev_f32(out, "out", contiguous=False, shape=(r, c))
    check(_lib.load().cer_copy_cols(ptr(x), x_ld, ptr(out), y_ld, r, c, current_stream()), "cer_copy_cols")
    return out


# ------------------------------------------------------------------ audio / text encoders
def logmel(pcm_int16, pad_samples, mel_matrix_f64, log_offset=0.01):
    """pcm [clips, S] int16 (16 kHz) -> log-mel [clips, frames, 64] float32."""
    if not (pcm_int16.is_cuda and pcm_int16.dtype == torch.int16 and pcm_int16.is_contiguous() and pcm_int16.dim() == 2):
        raise ValueError("pcm: expected a contiguous [clips, samples] int16 GPU tensor")
    if not (mel_matrix_f64.is_cuda and mel_matrix_f64.dtype == torch.float64 and tuple(mel_matrix_f64.shape) == (257, 64)
            and mel_matrix_f64.is_contiguous()):
        raise ValueError("mel matrix: expected a contiguous [257, 64] float64 GPU tensor")
    lib = _lib.load()
    clips, n = pcm_int16.shape
    frames = lib.cer_logmel_num_frames(n, pad_samples) if n > 0 and pad_samples >= 0 else 0
    if frames <= 0:
        raise ValueError(f"logmel: {n} samples + {pad_samples} of padding are shorter than one 400-sample frame")
    out = torch.empty((clips, frames, 64), device=pcm_int16.device, dtype=torch.float32)
    check(lib.cer_logmel_fwd(ptr(pcm_int16), clips, n, pad_samples, ptr(mel_matrix_f64), log_offset, ptr(out),
                             current_stream()), "cer_logmel_fwd")
    return out


def logmel_f64(samples_f64, mel_matrix_f64, log_offset=0.01):
    """samples [clips, S] float64 in [-1, 1) at 16 kHz (``resample_pcm``'s output) -> log-mel [clips, frames, 64] float32.
    No padding: the resampler has already read it."""
    if not (samples_f64.is_cuda and samples_f64.dtype == torch.float64 and samples_f64.is_contiguous()
            and samples_f64.dim() == 2):
        raise ValueError("samples: expected a contiguous [clips, samples] float64 GPU tensor")
    if not (mel_matrix_f64.is_cuda and mel_matrix_f64.dtype == torch.float64 and tuple(mel_matrix_f64.shape) == (257, 64)
            and mel_matrix_f64.is_contiguous()):
        raise ValueError("mel matrix: expected a contiguous [257, 64] float64 GPU tensor")
    lib = _lib.load()
    clips, n = samples_f64.shape
    frames = lib.cer_logmel_num_frames(n, 0) if n > 0 else 0
    if frames <= 0:
        raise ValueError(f"logmel_f64: {n} samples are shorter than one 400-sample frame")
    out = torch.empty((clips, frames, 64), device=samples_f64.device, dtype=torch.float32)
    check(lib.cer_logmel_f64_fwd(ptr(samples_f64), clips, n, ptr(mel_matrix_f64), log_offset, ptr(out), current_stream()),
          "cer_logmel_f64_fwd")
    return out


def resample_pcm(pcm_int16, channels_last, pad_samples, taps, L, M, n_out):
    """pcm [clips, S] int16, or interleaved [clips, S, C] with ``channels_last`` -> [clips, n_out] float64: the channel
    mean of pcm / 32768, ``pad_samples`` of edge padding, then out[n] = sum_j taps[(n M) mod L][j] * x[(n M) div L - J + j]
    with J = (T - 2) / 2 and zeros outside the padded signal.  ``taps`` [L, T] float64 on the GPU
    (``audio_backbone.resample_taps``); ``n_out`` is the caller's (``audio_backbone.resampled_length``)."""
    want = 3 if channels_last else 2
    if not (pcm_int16.is_cuda and pcm_int16.dtype == torch.int16 and pcm_int16.is_contiguous() and pcm_int16.dim() == want):
        raise ValueError("pcm: expected a contiguous int16 GPU tensor, [clips, samples, channels] with channels_last, "
                         "else [clips, samples]")
    L, M, n_out, pad_samples = int(L), int(M), int(n_out), int(pad_samples)
    if not (taps.is_cuda and taps.dtype == torch.float64 and taps.is_contiguous() and taps.dim() == 2
            and taps.shape[0] == L and taps.shape[1] >= 2 and taps.shape[1] % 2 == 0):
        raise ValueError("taps: expected a contiguous [L, T] float64 GPU tensor with T even")
    clips, n = pcm_int16.shape[:2]
    channels = pcm_int16.shape[2] if channels_last else 1
    if min(clips, n, channels, L, M, n_out) <= 0 or pad_samples < 0:
        raise ValueError(f"resample_pcm: empty input or bad sizes (pcm {tuple(pcm_int16.shape)}, L {L}, M {M}, "
                         f"n_out {n_out}, pad {pad_samples})")
    out = torch.empty((clips, n_out), device=pcm_int16.device, dtype=torch.float64)
    check(_lib.load().cer_resample_pcm(ptr(pcm_int16), clips, n, channels, pad_samples, ptr(taps), L, M, taps.shape[1],
                                       n_out, ptr(out), current_stream()), "cer_resample_pcm")
    return out


def frame_examples(logmel_t, starts, win=96):
    """[clips, frames, 64] -> [clips, n_examples, win, 64] at the given start rows.

    ``starts`` are HOST integers (a list, or a CPU integer tensor): the kernel reads ``logmel[starts[e] + f]`` unchecked,
    so every start is checked against [0, frames - win] here, before the upload and the launch, without touching the
    device.  A GPU tensor is refused: checking it would cost a synchronisation."""
    _dev_f32(logmel_t, "logmel")
    if logmel_t.dim() != 3 or logmel_t.shape[2] != 64:
        raise ValueError(f"logmel: expected [clips, frames, 64], got {tuple(logmel_t.shape)}")
    if isinstance(starts, torch.Tensor):
        if starts.is_cuda or starts.is_floating_point() or starts.dim() != 1:
            raise ValueError("starts: expected host integers (a list or a 1-D CPU integer tensor), so that they can be "
                             "bounds-checked without a device synchronisation")
        starts = starts.tolist()
    starts = [int(s) for s in starts]
    clips, frames, _ = logmel_t.shape
    win = int(win)
    if not starts or win <= 0 or win > frames:
        raise ValueError(f"frame_examples: need at least one start and 0 < win <= frames, got {len(starts)} starts, "
                         f"win {win}, {frames} frames")
    if min(starts) < 0 or max(starts) > frames - win:
        raise ValueError(f"frame_examples: starts must lie in [0, {frames - win}] ({frames} frames, win {win}), got "
                         f"[{min(starts)}, {max(starts)}]")
    n = len(starts)
    starts_i32 = torch.tensor(starts, dtype=torch.int32).to(logmel_t.device, non_blocking=True)
    out = torch.empty((clips, n, win, 64), device=logmel_t.device, dtype=torch.float32)
    check(_lib.load().cer_frame_examples(ptr(logmel_t), ptr(starts_i32), ptr(out), clips, frames, n, win,
                                         current_stream()), "cer_frame_examples")
    return out


def bert_embed_ln(ids, word, pos, typ, gamma, beta, eps=1e-12):
    if not (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2):
        raise ValueError("ids: expected a contiguous [B, S] int64 GPU tensor")
    for t, n in ((word, "word"), (pos, "pos"), (typ, "type"), (gamma, "gamma"), (beta, "beta")):
        _dev_f32(t, n)
    b, s = ids.shape
    hd = word.shape[1]
    y = torch.empty((b, s, hd), device=ids.device, dtype=torch.float32)
    check(_lib.load().cer_bert_embed_ln(ptr(ids), ptr(word), ptr(pos), ptr(typ), ptr(gamma), ptr(beta), ptr(y), b, s, hd,
                                        word.shape[0], pos.shape[0], eps, current_stream()), "cer_bert_embed_ln")
    return y


# bench.py sets this to a list to time the MFMA attention launches: (kind, algorithmic FLOPs, start event, end event)
ATTN_TRACE = None


def attention(q, k, v, out, batch, heads, sq, sk, d, q_strides, k_strides, v_strides, o_strides, scale, key_mask=None,
              lse=None):
    """Strided attention: element (b, s, h, :) at base + b*st[0] + s*st[1] + h*st[2].  q/k/v/out are
    (views into) float32 GPU buffers; only their data pointers are used."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (out, "out")):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise ValueError(f"{n}: expected a float32 GPU tensor")
    if key_mask is not None and not (key_mask.is_cuda and key_mask.dtype == torch.int32 and key_mask.is_contiguous()):
        raise ValueError("key_mask: expected a contiguous int32 GPU tensor [B, Sk]")
    LL3 = ctypes.c_longlong * 3
    if ATTN_TRACE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.load().cer_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(key_mask), ptr(out), ptr(lse), batch, heads, sq, sk, d,
                                        LL3(*q_strides), LL3(*k_strides), LL3(*v_strides), LL3(*o_strides), scale,
                                        current_stream()), "cer_attention_fwd")
    if ATTN_TRACE is not None:
        e1.record()
        ATTN_TRACE.append(("fwd" if sq * sk < (1 << 18) else f"fwd_{sq}x{sk}", 4.0 * batch * heads * sq * sk * d, e0, e1))
    return out


def attention_bwd(q, k, v, out, dout, lse, dq, dk, dv, batch, heads, sq, sk, d, q_strides, k_strides, v_strides,
                  o_strides, do_strides, dq_strides, dk_strides, dv_strides, scale, key_mask=None):
    """Gradients of ``attention`` written into dq/dk/dv (views allowed, strides given explicitly)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (dout, "dout"), (lse, "lse"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise ValueError(f"{n}: expected a float32 GPU tensor")
    LL3 = ctypes.c_longlong * 3
    delta = torch.empty_like(lse)
    if ATTN_TRACE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.load().cer_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(dout), ptr(lse), ptr(key_mask), ptr(delta),
                                        ptr(dq), ptr(dk), ptr(dv), batch, heads, sq, sk, d, LL3(*q_strides),
                                        LL3(*k_strides), LL3(*v_strides), LL3(*o_strides), LL3(*do_strides),
                                        LL3(*dq_strides), LL3(*dk_strides), LL3(*dv_strides), scale, current_stream()),
          "cer_attention_bwd")
    if ATTN_TRACE is not None:
        e1.record()
        ATTN_TRACE.append(("bwd" if sq * sk < (1 << 18) else f"bwd_{sq}x{sk}", 8.0 * batch * heads * sq * sk * d, e0, e1))


def add_inplace(y, x):
    _dev_f32(y, "y")
    _dev_f32(x, "x")
    check(_lib.load().cer_add_inplace(ptr(y), ptr(x), y.numel(), current_stream()), "cer_add_inplace")
    return y


# ------------------------------------------------------------------ streaming TCN (csrc/tcn_stream.hip)
STREAM_TRACE = None   # a list collects (entry point, weight bytes read) per launch


def _ring(t, name, channels=None):
    """A ring [S, R, C]: contiguous float32 on the GPU.  Returns (S, R, C)."""
    _dev_f32(t, name)
    shape = tuple(t.shape)
    if len(shape) != 3 or (channels is not None and shape[2] != channels):
        raise ValueError(f"{name}: expected a ring [S, R, {channels if channels is not None else 'C'}], got {shape}")
    return shape


def pack_tcn_stream_weight(w_oik):
    """Conv1d filter [Cout, Cin, k] -> the streaming kernel's [Cout4, k, Cin4] (channel counts rounded up to a multiple of 4,
    zero padding).  A layout change only; done once per weight."""
    _dev_f32(w_oik, "w", contiguous=False)
    if w_oik.dim() != 3:
        raise ValueError(f"w: expected [Cout, Cin, k], got {tuple(w_oik.shape)}")
    cout, cin, k = w_oik.shape
    out = torch.zeros((-(-cout // 4) * 4, k, -(-cin // 4) * 4), device=w_oik.device, dtype=torch.float32)
    out[:cout, :, :cin] = w_oik.detach().permute(0, 2, 1)
    return out


def tcn_stream_append(rows, ring, head):
    """ring[s, (head + i) % R, :] = rows[s, i, :]: ``rows`` [S, c, C] dense, ``ring`` [S, R, C]."""
    s, r, ch = _ring(ring, "ring")
    _dev_f32(rows, "rows")
    if rows.dim() != 3 or rows.shape[0] != s or rows.shape[2] != ch or rows.shape[1] < 1:
        raise ValueError(f"rows: expected [{s}, c, {ch}], got {tuple(rows.shape)}")
    check(_lib.load().cer_tcn_stream_append(ptr(rows), ptr(ring), s, rows.shape[1], ch, r, int(head), current_stream()),
          "cer_tcn_stream_append")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("append", 0))


def _addr(t):
    """``ptr`` as a plain int (the argtypes make the void *): a streamed push is bound by the host issuing its launches."""
    return None if t is None else t.data_ptr()


def _stream_conv(name, d, table, s, cin, rows, ring, w_packed, bias, res_ring, res_w, res_bias, out_ring, out_dense):
    """What ``tcn_stream_conv`` and ``tcn_stream_conv_rows`` share, which is all that does not depend on how a row finds its
    stream and position: the tensor checks, Cout and the residual and output rings of the entry's descriptor ``d``, the weight
    bytes and the one launch.  ``table``: the pointers that follow ``d`` in the call; ``s``, ``cin``: of the checked ``ring``;
    ``rows``: how many ``out_dense`` must have."""
    _dev_f32(bias, "bias")
    d.Cout = cout = bias.shape[0]
    cout4 = (cout + 3) & ~3   # the packed filters' channel counts: rounded up to a multiple of 4
    _dev_f32(w_packed, "w_packed", shape=(cout4, d.k, (cin + 3) & ~3))
    wbytes = w_packed.numel() * 4
    if res_ring is not None:
        rs, d.res_R, d.res_C = _ring(res_ring, "res_ring")
        if rs != s:
            raise ValueError(f"res_ring: expected {s} streams, got {rs}")
        if res_w is not None:
            _dev_f32(res_w, "res_w", shape=(cout4, 1, (d.res_C + 3) & ~3))
            _dev_f32(res_bias, "res_bias", shape=(cout,))
            if res_bias is None:
                raise ValueError("res_bias: the projection needs its bias")
            wbytes += res_w.numel() * 4
        elif d.res_C != cout:
            raise ValueError(f"res_ring: {d.res_C} channels for Cout = {cout} and no projection")
    elif res_w is not None or res_bias is not None:
        raise ValueError("res_w / res_bias without res_ring")
    if out_ring is None and out_dense is None:
        raise ValueError(f"tcn_stream_{name}: no output")
    if out_ring is not None:
        os_, d.out_R, _ = _ring(out_ring, "out_ring", cout)
        if os_ != s:
            raise ValueError(f"out_ring: expected {s} streams, got {os_}")
    _dev_f32(out_dense, "out_dense", shape=(rows, cout))
    entry = "cer_tcn_stream_" + name
    check(getattr(_lib.load(), entry)(ctypes.byref(d), *table, ring.data_ptr(), w_packed.data_ptr(), bias.data_ptr(),
                                      _addr(res_ring), _addr(res_w), _addr(res_bias), _addr(out_ring), _addr(out_dense),
                                      current_stream()), entry)
    if STREAM_TRACE is not None:
        STREAM_TRACE.append((name, wbytes))


def tcn_stream_conv(ring, head, c, w_packed, bias, k, dil, *, res_ring=None, res_head=0, res_w=None, res_bias=None,
                    out_ring=None, out_head=0, out_dense=None, slope=LEAKY_SLOPE):
    """One conv of a streamed TemporalBlock over the ``c`` newest frames of ``ring`` [S, R, Cin] (written at ``head``):

      v = leaky(conv_k,dil(ring) + bias)                     without ``res_ring``
      v = leaky(leaky(conv_k,dil(ring) + bias) + res)        with it: res = the c newest frames of ``res_ring`` (at ``res_head``),
                                                             or their 1x1 projection ``res_w`` (packed) + ``res_bias``

    written to the c slots of ``out_ring`` [S, R', Cout] at ``out_head`` and / or to ``out_dense`` [S * c, Cout].
    ``w_packed``: ``pack_tcn_stream_weight`` of the [Cout, Cin, k] filter."""
    s, r, cin = _ring(ring, "ring")
    d = _lib.TcnStreamDesc(S=s, c=int(c), Cin=cin, k=int(k), dil=int(dil), R=r, head=int(head), res_head=int(res_head),
                           out_head=int(out_head), slope=float(slope))
    _stream_conv("conv", d, (), s, cin, s * int(c), ring, w_packed, bias, res_ring, res_w, res_bias, out_ring, out_dense)


def pow2_at_least(n):
    """The power of two >= n (1 for n <= 1): the length of every ring, so that a position is masked, not divided."""
    r = 1
    while r < n:
        r *= 2
    return r


ROW_POS_MOD = 1 << 30   # row positions travel modulo 2^30: every ring length divides it, so each launch's mask sees the same slot


def _stream_rows(positions, counts):
    """The rows of one ragged push as two lists of Python ints: (stream of row m, position of row m modulo 2^30)."""
    positions, counts = [int(p) for p in positions], [int(c) for c in counts]
    if len(positions) != len(counts):
        raise ValueError(f"stream_row_table: {len(positions)} positions for {len(counts)} counts")
    for s, (p, c) in enumerate(zip(positions, counts)):
        if c < 0 or p < 0:
            raise ValueError(f"stream_row_table: stream {s} has count {c} at position {p}: both must be >= 0")
    streams = [s for s, c in enumerate(counts) for _ in range(c)]
    return streams, [(p + i) % ROW_POS_MOD for p, c in zip(positions, counts) for i in range(c)]


def _upload_rows(positions, counts, device, payload=None, dtype=np.int32, cols=0, name="stream_row_table"):
    """The row table of ``_stream_rows`` and an optional per-row ``payload`` [M, cols] of ``dtype`` as ONE fresh int32 host
    array [payload | streams | positions] and one upload (no staging buffer an unfinished copy could still read).  The payload
    leads, so 8-byte values sit at the allocation's aligned start whatever M.
    Returns (row_stream [M], row_pos [M], the payload's int32 words or None), views of that tensor on ``device``."""
    streams, pos = _stream_rows(positions, counts)
    m, w = len(streams), 0
    if payload is not None:
        payload = np.ascontiguousarray(payload, dtype=dtype)
        if payload.shape != (m, cols):
            raise ValueError(f"{name}: expected one entry per row [{m}, {cols}], got {payload.shape}")
        w = payload.nbytes // 4
    host = np.empty(w + 2 * m, np.int32)
    host[w:] = streams + pos
    if w:
        host[:w] = payload.ravel().view(np.int32)
    table = torch.from_numpy(host).to(device)
    return table[w:w + m], table[w + m:], None if payload is None else table[:w]


def stream_row_table(positions, counts, device):
    """The row table of one ragged push: stream s brings ``counts[s]`` frames, the first at position ``positions[s]`` (frames
    that stream has been pushed so far).  Returns (row_stream, row_pos), int32 [M] each on ``device``: rows stream-major in
    ascending stream order, a stream's frames in time order, positions modulo 2^30; a stream with count 0 has no row.
    Built from Python ints and uploaded in one fresh tensor per call (``_upload_rows``)."""
    return _upload_rows(positions, counts, device)[:2]


DECISION_FIELDS = 6   # stream, count, offset, position, frames (low word), frames (high word)


def decision_segment_table(segments, device):
    """The table of one ``decision_stream_push`` (or ``decision_stream_read``): ``segments`` = (stream, count, offset into the
    packed rows, ring position, frames since reset) per entry, Python ints -> int32 [6, A] on ``device``: the first three as
    they are, the position modulo 2^30, the frames as a 64-bit value split into its low and high 32-bit words (each stored as
    the int32 with those bits).  One fresh tensor per call, like ``stream_row_table``."""
    cols = []
    for s, count, off, pos, frames in segments:
        s, count, off, pos, frames = int(s), int(count), int(off), int(pos), int(frames)
        if count < 0 or pos < 0 or not 0 <= frames < (1 << 63) or not 0 <= off < (1 << 31) or not -(1 << 31) <= s < (1 << 31) \
                or count >= (1 << 31):
            raise ValueError(f"decision_segment_table: segment of stream {s}: count {count}, offset {off}, position {pos}, "
                             f"frames {frames}")
        lo, hi = frames & 0xffffffff, frames >> 32
        cols.append((s, count, off, pos % ROW_POS_MOD, lo - (1 << 32) if lo >= (1 << 31) else lo, hi))
    if not cols:
        raise ValueError("decision_segment_table: no segment")
    return torch.tensor([[c[f] for c in cols] for f in range(DECISION_FIELDS)], dtype=torch.int32, device=device)


def _row_table(row_stream, row_pos, ring):
    """Both tables int32, contiguous, one-dimensional, on the ring's device and of one length M >= 1.  Returns M."""
    for t, n in ((row_stream, "row_stream"), (row_pos, "row_pos")):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == ring.device and t.dtype == torch.int32 and t.is_contiguous()
                and t.dim() == 1):
            raise ValueError(f"{n}: expected a contiguous int32 vector on the GPU of the ring ({ring.device}), got "
                             f"{(t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t)}")
    if row_stream.shape[0] != row_pos.shape[0] or row_stream.shape[0] < 1:
        raise ValueError(f"row_stream / row_pos: expected one length M >= 1, got {row_stream.shape[0]} and {row_pos.shape[0]}")
    return row_stream.shape[0]


def tcn_stream_append_rows(rows, ring, row_stream, row_pos, max_count):
    """ring[row_stream[m], row_pos[m] % R, :] = rows[m, :]: ``rows`` [M, C] dense, ``ring`` [S, R, C], the tables of
    ``stream_row_table``; ``max_count``: the most rows any one stream has in them."""
    s, r, ch = _ring(ring, "ring")
    m = _row_table(row_stream, row_pos, ring)
    _dev_f32(rows, "rows")
    if rows.dim() != 2 or rows.shape[0] != m or rows.shape[1] != ch:
        raise ValueError(f"rows: expected [{m}, {ch}], got {tuple(rows.shape)}")
    check(_lib.load().cer_tcn_stream_append_rows(ptr(rows), ptr(ring), ptr(row_stream), ptr(row_pos), s, m, int(max_count), ch, r,
                                                 current_stream()), "cer_tcn_stream_append_rows")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("append_rows", 0))


def tcn_stream_conv_rows(ring, row_stream, row_pos, max_count, w_packed, bias, k, dil, *, res_ring=None, res_w=None,
                         res_bias=None, out_ring=None, out_dense=None, slope=LEAKY_SLOPE):
    """``tcn_stream_conv`` over the M rows of a row table instead of the c newest frames of every stream: row m is the frame
    of stream ``row_stream[m]`` at position ``row_pos[m]`` in ``ring``, ``res_ring`` and ``out_ring`` alike (each masks the
    position with its own length); ``out_dense`` is [M, Cout].  A stream's rows are consecutive positions, at most
    ``max_count`` of them.  The same bits as the lockstep launch gives the same frames."""
    s, r, cin = _ring(ring, "ring")
    m = _row_table(row_stream, row_pos, ring)
    d = _lib.TcnStreamRowsDesc(S=s, M=m, max_count=int(max_count), Cin=cin, k=int(k), dil=int(dil), R=r, slope=float(slope))
    _stream_conv("conv_rows", d, (ptr(row_stream), ptr(row_pos)), s, cin, m, ring, w_packed, bias, res_ring, res_w, res_bias,
                 out_ring, out_dense)


# ------------------------------------------------------------------ token rows -> frame rows (csrc/text_spread.hip)
def text_spread_tables(segments, out_rows, tok_rows):
    """The two tables of one ``text_spread_rows`` as Python ints, checked: ``segments`` = (out_first, n_frames, token_rows) per
    entry -> ([(out_first, n_frames, n_tokens, index_first)], the token rows of all segments in order).  Output ranges are
    disjoint and inside [0, out_rows), every token row is inside [0, tok_rows).  No GPU."""
    table, index, spans = [], [], []
    for g, seg in enumerate(segments):
        try:
            first, frames, rows = seg
            rows = list(rows)
        except (TypeError, ValueError):
            raise ValueError(f"text_spread_rows: segment {g}: expected (out_first, n_frames, token_rows), got {seg!r}") from None
        for v in (first, frames, *rows):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"text_spread_rows: segment {g}: {v!r} is not an int")
        first, frames = int(first), int(frames)
        if frames < 1 or first < 0 or first + frames > out_rows:
            raise ValueError(f"text_spread_rows: segment {g}: frames [{first}, {first + frames}) outside [0, {out_rows}) or empty")
        for t in rows:
            if not 0 <= t < tok_rows:
                raise ValueError(f"text_spread_rows: segment {g}: token row {t} outside [0, {tok_rows})")
        table.append((first, frames, len(rows), len(index)))
        index += [int(t) for t in rows]
        spans.append((first, first + frames, g))
    if not table:
        raise ValueError("text_spread_rows: no segment")
    spans.sort()
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        if start < end:
            raise ValueError(f"text_spread_rows: segments {a} and {b} overlap at output row {start}")
    return table, index


def text_spread_rows(tok, segments, out_rows, out=None):
    """Token rows of one or more sentences -> the rows of spans of frames (speech.py:690-738), one launch.  ``tok`` [T, hidden]
    fp32; ``segments``: (out_first, n_frames, token_rows) per entry, Python ints: frame i of the n_frames output rows from
    out_first shows row ``token_rows[j(i)]`` of ``tok``, the frames divided into min(len(token_rows), n_frames) contiguous
    blocks of which the first n_frames % n are one longer (``feature_extractor.align_tokens_to_frames``), or zeros when
    ``token_rows`` is empty.  Returns ``out`` [out_rows, hidden]; rows no segment covers are zeros in a fresh ``out`` and stay
    as they are in a caller's.  Both tables travel as one fresh int32 tensor per call [segments | index]."""
    _dev_f32(tok, "tok")
    out_rows = int(out_rows)
    if tok.dim() != 2 or tok.shape[0] < 1 or tok.shape[1] % 4 or tok.shape[1] < 4:
        raise ValueError(f"tok: expected [T >= 1, hidden] with hidden a multiple of 4, got {tuple(tok.shape)}")
    if out_rows < 1:
        raise ValueError(f"out_rows = {out_rows}: must be >= 1")
    if out is not None:
        _dev_f32(out, "out")
        if tuple(out.shape) != (out_rows, tok.shape[1]) or out.device != tok.device:
            raise ValueError(f"out: expected [{out_rows}, {tok.shape[1]}] on {tok.device}, got {tuple(out.shape)} on {out.device}")
    table, index = text_spread_tables(segments, out_rows, tok.shape[0])
    g = len(table)
    host = np.zeros(4 * g + max(len(index), 1), np.int32)   # a lone 0 when no segment has a token: the entry wants n_index >= 1
    host[:4 * g] = np.asarray(table, np.int64).ravel()
    host[4 * g:4 * g + len(index)] = index
    dev = torch.from_numpy(host).to(tok.device)
    if out is None:
        out = torch.zeros((out_rows, tok.shape[1]), device=tok.device, dtype=torch.float32)
    check(_lib.load().cer_text_spread_rows(ptr(tok), tok.shape[0], tok.shape[1], ptr(dev[:4 * g]), g, ptr(dev[4 * g:]),
                                           host.shape[0] - 4 * g, ptr(out), out_rows, current_stream()), "cer_text_spread_rows")
    return out


# ------------------------------------------------------------------ standardised vggish / bert rows (csrc/feature_norm.hip)
FEATURE_NORM_MAX_C = 1 << 20


def _feature_rows(t, name):
    """A dense [M >= 1, C] float32 GPU tensor with C in the kernels' range and M * C < 2^31.  Returns (M, C)."""
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
    _dev_f32(t, name)
    if t.dim() != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= FEATURE_NORM_MAX_C or t.numel() >= (1 << 31):
        raise ValueError(f"{name}: expected [M >= 1, 1 <= C <= {FEATURE_NORM_MAX_C}] with M * C < 2^31, got {tuple(t.shape)}")
    return t.shape[0], t.shape[1]


def feature_moments_update(rows, acc):
    """acc[0] += rows.sum(0), acc[1] += (rows ** 2).sum(0) in float64, the adds of a column in row order: ``rows`` [M, C]
    float32, ``acc`` [2, C] float64 on the same GPU, updated in place.  The bits of ``acc`` depend on the sequence of rows
    only, not on how it was split over calls.  Returns ``acc``."""
    m, c = _feature_rows(rows, "rows")
    if not (torch.is_tensor(acc) and acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous()
            and tuple(acc.shape) == (2, c) and acc.device == rows.device):
        raise ValueError(f"acc: expected a contiguous float64 [2, {c}] on {rows.device}, got "
                         f"{(acc.dtype, acc.device, tuple(acc.shape)) if torch.is_tensor(acc) else type(acc)}")
    check(_lib.load().cer_feature_moments_update(ptr(rows), m, c, ptr(acc), current_stream()), "cer_feature_moments_update")
    return acc


def standardize_rows(x, mean, std, out=None):
    """(x - mean) / std per column in float32, one subtraction and one correctly rounded division: ``torch.equal`` with
    ``x.sub(mean).div(std)`` (torchvision's Normalize).  ``x`` [M, C] float32 with C % 4 == 0; ``mean``, ``std`` [C] float32 on
    the same GPU; ``out``: where to write, ``x`` itself for in place, a fresh tensor by default.  Returns ``out``."""
    m, c = _feature_rows(x, "x")
    if c % 4:
        raise ValueError(f"x: C = {c} is not a multiple of 4 (the rows move as float4)")
    for t, n in ((mean, "mean"), (std, "std")):
        if not torch.is_tensor(t):
            raise ValueError(f"{n}: expected a tensor, got {type(t).__name__}")
        _dev_f32(t, n, shape=(c,))
        if t.device != x.device:
            raise ValueError(f"{n}: on {t.device}, x on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    else:
        if not torch.is_tensor(out):
            raise ValueError(f"out: expected a tensor, got {type(out).__name__}")
        _dev_f32(out, "out", shape=(m, c))
        if out.device != x.device:
            raise ValueError(f"out: on {out.device}, x on {x.device}")
        if out.data_ptr() != x.data_ptr() and out.data_ptr() < x.data_ptr() + 4 * m * c and x.data_ptr() < out.data_ptr() + 4 * m * c:
            raise ValueError("out: overlaps x without being x")
    for t, n in ((x, "x"), (mean, "mean"), (std, "std"), (out, "out")):
        if t.data_ptr() % 16:
            raise ValueError(f"{n}: storage is not 16-byte aligned (the rows move as float4)")
    check(_lib.load().cer_standardize_rows(ptr(x), m, c, ptr(mean), ptr(std), ptr(out), current_stream()), "cer_standardize_rows")
    return out


# ------------------------------------------------------------------ the window rule on live streams (csrc/window_stream.hip)
def window_stitch_tables(rows, done, tail, streams, slots, window, hop):
    """The tables of one ``window_stitch_stream`` as Python ints, checked: ``rows`` = (stream, frame) per output row, ``done``
    [S] the regular windows each stream has run, ``tail`` [S] the start of its tail (or short) window, -1 for none ->
    (row streams, row frames).  Every row's stream is inside [0, S) and its frame inside [0, 2^31 - W); no regular window that
    covers a row has left the ring (windows done - (slots - 1) .. done - 1 are in it) and at least one live window covers it.
    No GPU."""
    done, tail = [int(d) for d in done], [int(t) for t in tail]
    if len(done) != streams or len(tail) != streams:
        raise ValueError(f"window_stitch_stream: expected {streams} window counts and tail starts, got {len(done)} and {len(tail)}")
    for s, (d, t) in enumerate(zip(done, tail)):
        if d < 0 or t < -1 or max(d * hop, t) >= (1 << 31) - window:
            raise ValueError(f"window_stitch_stream: stream {s}: {d} windows done, tail start {t}")
    if not rows:
        raise ValueError("window_stitch_stream: no row")
    rs, rf = [], []
    for p, (s, f) in enumerate(rows):
        s, f = int(s), int(f)
        if not 0 <= s < streams or not 0 <= f < (1 << 31) - window:
            raise ValueError(f"window_stitch_stream: row {p}: frame {f} of stream {s} ({streams} streams)")
        first = max((f - window) // hop + 1, 0)         # the lowest regular window that covers f
        if first < done[s] - (slots - 1):
            raise ValueError(f"window_stitch_stream: row {p}: window {first} of stream {s} covers frame {f} and has left the "
                             f"ring of {slots - 1} regular slots ({done[s]} windows done)")
        if not (first < done[s] or 0 <= f - tail[s] < window and tail[s] >= 0):
            raise ValueError(f"window_stitch_stream: row {p}: no live window of stream {s} covers frame {f}")
        rs.append(s)
        rf.append(f)
    return rs, rf


def window_stitch_stream(wring, hop, rows, done, tail, out=None):
    """The frames ``rows`` = [(stream, frame)] stitched from the ring ``wring`` [S, K, W, C] of each stream's last window
    outputs (regular window i in slot i % (K - 1), the tail or short window in slot K - 1): ``out`` [P, C], each element the
    bits ``eval_device.stitch_windows`` gives the same window outputs (a float32 sum from 0 in ascending window start, the
    tail last, one division by the count).  ``done`` / ``tail``: per stream, the regular windows run so far and the tail's
    start (-1: none).  All four tables are Python ints, checked on the host (``window_stitch_tables``) and uploaded as ONE
    fresh int32 tensor [row streams | row frames | done | tail]."""
    _dev_f32(wring, "wring")
    if wring.dim() != 4 or min(wring.shape) < 1 or wring.shape[1] < 2:
        raise ValueError(f"wring: expected [S, K >= 2, W, C], got {tuple(wring.shape)}")
    s, k, w, c = wring.shape
    hop = int(hop)
    if not 1 <= hop <= w:
        raise ValueError(f"hop = {hop}: must be in 1 .. W = {w}")
    rs, rf = window_stitch_tables(rows, done, tail, s, k, w, hop)
    p = len(rs)
    if out is None:
        out = torch.empty((p, c), device=wring.device, dtype=torch.float32)
    else:
        _dev_f32(out, "out", shape=(p, c))
        if out.device != wring.device:
            raise ValueError(f"out: on {out.device}, the ring on {wring.device}")
    host = np.asarray(rs + rf + [int(d) for d in done] + [int(t) for t in tail], np.int32)
    dev = torch.from_numpy(host).to(wring.device)
    check(_lib.load().cer_window_stitch_stream(ptr(wring), s, k, w, c, hop, ptr(dev[:p]), ptr(dev[p:2 * p]), p,
                                               ptr(dev[2 * p:2 * p + s]), ptr(dev[2 * p + s:]), ptr(out), current_stream()),
          "cer_window_stitch_stream")
    return out


# ------------------------------------------------------------------ streaming log-mel (csrc/logmel_stream.hip)
def logmel_stream_tables(segments, rows, examples, device):
    """The three tables of one streamed log-mel push, from Python ints, uploaded as ONE fresh int32 tensor (one H2D copy, no
    staging buffer an unfinished copy could still read):

      segments  (stream, position of the first new sample, count, offset into the packed input or None = repeat the sample
                before the position ``count`` times)                                                   -> int32 [4, A]
      rows      (stream, position of the row's first sample, row number)                               -> int32 [3, N]
      examples  (stream, start row)                                                                    -> int32 [2, E]

    Positions and row numbers are unbounded Python ints and are reduced modulo 2^30 here and only here.  Returns the three
    views; an empty list gives None."""
    cols = []
    for s, pos, count, off in segments:
        s, pos, count = int(s), int(pos), int(count)
        off = -1 if off is None else int(off)
        if pos < 0 or count < 1 or not -1 <= off < (1 << 31) - 1:
            raise ValueError(f"logmel_stream_tables: segment of stream {s}: position {pos}, count {count}, offset {off}")
        cols.append((s, pos % ROW_POS_MOD, count, off))
    seg = [c[f] for f in range(4) for c in cols]
    row = [(int(s), int(pos) % ROW_POS_MOD, int(r) % ROW_POS_MOD) for s, pos, r in rows]
    ex = [(int(s), int(start) % ROW_POS_MOD) for s, start in examples]
    flat = seg + [c[f] for f in range(3) for c in row] + [c[f] for f in range(2) for c in ex]
    for v in flat:
        if not -(1 << 31) <= v < (1 << 31):
            raise ValueError(f"logmel_stream_tables: {v} does not fit an int32")
    table = torch.tensor(flat, dtype=torch.int32, device=device)
    a, n, e = 4 * len(cols), 3 * len(row), 2 * len(ex)
    return (table[:a].view(4, -1) if a else None, table[a:a + n].view(3, -1) if n else None,
            table[a + n:a + n + e].view(2, -1) if e else None)


def _stream_table(t, name, fields, like):
    """An int32 table [fields, n >= 1], contiguous, on the device of ``like``.  Returns n."""
    if not (torch.is_tensor(t) and t.is_cuda and t.device == like.device and t.dtype == torch.int32 and t.is_contiguous()
            and t.dim() == 2 and t.shape[0] == fields and t.shape[1] >= 1):
        raise ValueError(f"{name}: expected a contiguous int32 [{fields}, n >= 1] table on the GPU of the ring ({like.device}), "
                         f"got {(t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t)}")
    return t.shape[1]


def _sample_ring(t):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int16 and t.is_contiguous() and t.dim() == 2):
        raise ValueError("ring: expected a contiguous [S, Rs] int16 GPU tensor")
    return t.shape


def _logmel_ring(t):
    _dev_f32(t, "logmel_ring")
    if t.dim() != 3 or t.shape[2] != 64:
        raise ValueError(f"logmel_ring: expected [S, Rm, 64], got {tuple(t.shape)}")
    return t.shape[0], t.shape[1]


def logmel_stream_append(packed, segments, max_count, ring):
    """Write the new int16 samples ``packed`` [M >= 1] of a push into the sample ring [S, Rs] as the segment table says
    (``logmel_stream_tables``); ``max_count``: the largest count in it."""
    s, rs = _sample_ring(ring)
    if not (torch.is_tensor(packed) and packed.is_cuda and packed.device == ring.device and packed.dtype == torch.int16
            and packed.is_contiguous() and packed.dim() == 1 and packed.shape[0] >= 1):
        raise ValueError("packed: expected a contiguous int16 vector of at least one sample on the GPU of the ring")
    a = _stream_table(segments, "segments", 4, ring)
    check(_lib.load().cer_logmel_stream_append(ptr(packed), packed.shape[0], ptr(segments), a, int(max_count), ptr(ring), s, rs,
                                               current_stream()), "cer_logmel_stream_append")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("logmel_append", 0))


def logmel_stream_rows(ring, rows, mel_matrix_f64, logmel_ring, log_offset=0.01):
    """One log-mel row per entry of the row table, from 400 samples of the sample ring [S, Rs] into the log-mel ring
    [S, Rm, 64]: the bits ``logmel`` gives the same samples."""
    s, rs = _sample_ring(ring)
    sm, rm = _logmel_ring(logmel_ring)
    if sm != s or logmel_ring.device != ring.device:
        raise ValueError(f"logmel_ring: expected {s} streams on {ring.device}, got {sm} on {logmel_ring.device}")
    if not (mel_matrix_f64.is_cuda and mel_matrix_f64.dtype == torch.float64 and tuple(mel_matrix_f64.shape) == (257, 64)
            and mel_matrix_f64.is_contiguous() and mel_matrix_f64.device == ring.device):
        raise ValueError("mel matrix: expected a contiguous [257, 64] float64 tensor on the GPU of the ring")
    n = _stream_table(rows, "rows", 3, ring)
    check(_lib.load().cer_logmel_stream_rows(ptr(ring), s, rs, ptr(rows), n, ptr(mel_matrix_f64), log_offset, ptr(logmel_ring),
                                             rm, current_stream()), "cer_logmel_stream_rows")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("logmel_rows", 0))


def logmel_stream_examples(logmel_ring, examples, win=96):
    """Gather ``win`` rows of the log-mel ring [S, Rm, 64] per entry of the example table -> [E, win, 64]."""
    s, rm = _logmel_ring(logmel_ring)
    e = _stream_table(examples, "examples", 2, logmel_ring)
    win = int(win)
    if not 1 <= win <= rm:
        raise ValueError(f"logmel_stream_examples: win = {win} outside 1 .. Rm = {rm}")
    out = torch.empty((e, win, 64), device=logmel_ring.device, dtype=torch.float32)
    check(_lib.load().cer_logmel_stream_examples(ptr(logmel_ring), s, rm, ptr(examples), e, win, ptr(out), current_stream()),
          "cer_logmel_stream_examples")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("logmel_examples", 0))
    return out


# ------------------------------------------------------------------ streaming resampler (csrc/logmel_stream.hip)
def resample_stream_tables(mix, outputs, rows, examples, device):
    """The four tables of one resampled push, from Python ints, uploaded as ONE fresh int32 tensor like
    ``logmel_stream_tables``:

      mix       (stream, position of the first new input frame, count, offset in frames into the packed input or None =
                repeat the sample before the position)                                                  -> int32 [4, A]
      outputs   (stream, first output n0, count, r0, q0, inputs the stream has) with q0, r0 = divmod(n0 M, L): the kernel
                gets n0 and q0 as ring positions and the stream's valid inputs [0, inputs) as the range [-q0, inputs - q0)
                relative to q0                                                                          -> int32 [7, B]
      rows      (stream, position of the row's first 16 kHz sample, row number)                         -> int32 [3, N]
      examples  (stream, start row)                                                                     -> int32 [2, E]

    Positions are unbounded Python ints and are reduced modulo 2^30 here and only here; the two ends of the valid range are
    clamped to +-2^30, further than any launch reads.  Returns the four views; an empty list gives None."""
    mcols = []
    for s, pos, count, off in mix:
        s, pos, count = int(s), int(pos), int(count)
        off = -1 if off is None else int(off)
        if pos < 0 or count < 1 or not -1 <= off < (1 << 31) - 1:
            raise ValueError(f"resample_stream_tables: mix segment of stream {s}: position {pos}, count {count}, offset {off}")
        mcols.append((s, pos % ROW_POS_MOD, count, off))
    ocols = []
    for s, n0, count, r0, q0, inputs in outputs:
        s, n0, count, r0, q0, inputs = int(s), int(n0), int(count), int(r0), int(q0), int(inputs)
        if n0 < 0 or count < 1 or r0 < 0 or q0 < 0 or inputs < 0:
            raise ValueError(f"resample_stream_tables: output segment of stream {s}: n0 {n0}, count {count}, r0 {r0}, q0 {q0}, "
                             f"inputs {inputs}")
        lo, hi = (min(max(v, -ROW_POS_MOD), ROW_POS_MOD) for v in (-q0, inputs - q0))
        ocols.append((s, n0 % ROW_POS_MOD, count, r0, q0 % ROW_POS_MOD, lo, hi))
    row = [(int(s), int(pos) % ROW_POS_MOD, int(r) % ROW_POS_MOD) for s, pos, r in rows]
    ex = [(int(s), int(start) % ROW_POS_MOD) for s, start in examples]
    flat = []
    for cols, fields in ((mcols, 4), (ocols, 7), (row, 3), (ex, 2)):
        flat += [c[f] for f in range(fields) for c in cols]
    for v in flat:
        if not -(1 << 31) <= v < (1 << 31):
            raise ValueError(f"resample_stream_tables: {v} does not fit an int32")
    table = torch.tensor(flat, dtype=torch.int32, device=device)
    views, at = [], 0
    for cols, fields in ((mcols, 4), (ocols, 7), (row, 3), (ex, 2)):
        n = fields * len(cols)
        views.append(table[at:at + n].view(fields, -1) if n else None)
        at += n
    return tuple(views)


def _f64_ring(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 2):
        raise ValueError(f"{name}: expected a contiguous [S, R] float64 GPU tensor")
    return t.shape


def resample_stream_append(packed, segments, max_count, history, in_ring):
    """Mix the new int16 frames ``packed`` ([M >= 1] mono or interleaved [M, C]) of a push down into the mixed-input ring
    [S, Rin] float64 as the mix table says (``resample_stream_tables``); ``max_count``: the largest count in it;
    ``history``: the inputs before the new ones that are still needed (T - 1)."""
    s, rin = _f64_ring(in_ring, "in_ring")
    if not (torch.is_tensor(packed) and packed.is_cuda and packed.device == in_ring.device and packed.dtype == torch.int16
            and packed.is_contiguous() and packed.dim() in (1, 2) and packed.shape[0] >= 1 and packed.numel() >= 1):
        raise ValueError("packed: expected a contiguous int16 [M] or [M, C] tensor of at least one frame on the GPU of the ring")
    channels = packed.shape[1] if packed.dim() == 2 else 1
    a = _stream_table(segments, "segments", 4, in_ring)
    check(_lib.load().cer_resample_stream_append(ptr(packed), packed.shape[0], channels, ptr(segments), a, int(max_count),
                                                 int(history), ptr(in_ring), s, rin, current_stream()),
          "cer_resample_stream_append")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("resample_append", 0))


def resample_stream_outputs(in_ring, segments, max_count, taps, L, M, out_ring):
    """The 16 kHz samples the output table names, from the mixed-input ring [S, Rin] into the sample ring [S, Rs] (both
    float64): the bits ``resample_pcm`` gives the same inputs.  ``taps`` [L, T] float64; ``max_count``: the largest count."""
    s, rin = _f64_ring(in_ring, "in_ring")
    so, rs = _f64_ring(out_ring, "out_ring")
    if so != s or out_ring.device != in_ring.device:
        raise ValueError(f"out_ring: expected {s} streams on {in_ring.device}, got {so} on {out_ring.device}")
    L, M = int(L), int(M)
    if not (taps.is_cuda and taps.dtype == torch.float64 and taps.is_contiguous() and taps.dim() == 2 and L >= 1
            and taps.shape[0] == L and taps.shape[1] >= 2 and taps.shape[1] % 2 == 0 and taps.device == in_ring.device):
        raise ValueError("taps: expected a contiguous [L, T] float64 tensor with T even on the GPU of the rings")
    b = _stream_table(segments, "segments", 7, in_ring)
    check(_lib.load().cer_resample_stream_outputs(ptr(in_ring), s, rin, ptr(segments), b, int(max_count), ptr(taps), L, M,
                                                  taps.shape[1], ptr(out_ring), rs, current_stream()),
          "cer_resample_stream_outputs")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("resample_outputs", 0))


def logmel_stream_rows_f64(ring, rows, mel_matrix_f64, logmel_ring, log_offset=0.01):
    """``logmel_stream_rows`` on the float64 16 kHz ring [S, Rs]: the bits ``logmel_f64`` gives the same samples."""
    s, rs = _f64_ring(ring, "ring")
    sm, rm = _logmel_ring(logmel_ring)
    if sm != s or logmel_ring.device != ring.device:
        raise ValueError(f"logmel_ring: expected {s} streams on {ring.device}, got {sm} on {logmel_ring.device}")
    if not (mel_matrix_f64.is_cuda and mel_matrix_f64.dtype == torch.float64 and tuple(mel_matrix_f64.shape) == (257, 64)
            and mel_matrix_f64.is_contiguous() and mel_matrix_f64.device == ring.device):
        raise ValueError("mel matrix: expected a contiguous [257, 64] float64 tensor on the GPU of the ring")
    n = _stream_table(rows, "rows", 3, ring)
    check(_lib.load().cer_logmel_stream_rows_f64(ptr(ring), s, rs, ptr(rows), n, ptr(mel_matrix_f64), log_offset,
                                                 ptr(logmel_ring), rm, current_stream()), "cer_logmel_stream_rows_f64")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("logmel_rows_f64", 0))


# ------------------------------------------------------------------ streaming frame transform (csrc/frames_stream.hip)
def stream_pair_table(pairs, device):
    """The row table of explicit rows: ``pairs`` = (stream, position) per row, in the caller's order, Python ints of any size
    -> (row_stream, row_pos) like ``stream_row_table``: int32 [M] each, positions modulo 2^30, one fresh upload."""
    pairs = [(int(s), int(p)) for s, p in pairs]
    for s, p in pairs:
        if p < 0 or not -(1 << 31) <= s < (1 << 31):
            raise ValueError(f"stream_pair_table: row (stream {s}, position {p}): a position must be >= 0, a stream an int32")
    table = torch.tensor([[s for s, _ in pairs], [p % ROW_POS_MOD for _, p in pairs]], dtype=torch.int32,
                         device=device).view(2, len(pairs))
    return table[0], table[1]


def _u8_ring(t, crop=None):
    """The frame ring [S, Rf, crop, crop, 3]: contiguous uint8 on the GPU.  Returns (S, Rf, crop)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 5
            and t.shape[2] == t.shape[3] and t.shape[4] == 3 and (crop is None or t.shape[2] == crop)):
        raise ValueError(f"u8ring: expected a contiguous uint8 [S, Rf, {crop or 'crop'}, {crop or 'crop'}, 3] GPU tensor, got "
                         f"{(t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t)}")
    return t.shape[0], t.shape[1], t.shape[2]


def _i32_table(t, name, shape, like):
    if not (torch.is_tensor(t) and t.is_cuda and t.device == like.device and t.dtype == torch.int32 and t.is_contiguous()
            and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous int32 {list(shape)} tensor on the GPU of the ring ({like.device}), got "
                         f"{(t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t)}")


def _yuv_frames(frames, yuv, like):
    """The check of 4:2:0 frames that the ``yuv=`` forms of the frame wrappers share: ``frames`` uint8 [n, H * 3 / 2, W] of
    an H x W picture, H and W even, on the GPU of ``like``; ``yuv`` the ``cer_yuv420`` of ``frames.yuv_desc``.
    Returns (n, H, W)."""
    from .frames import yuv_picture
    if not isinstance(yuv, _lib.Yuv420Desc):
        raise ValueError(f"yuv: expected the descriptor of frames.yuv_desc, got {type(yuv).__name__}")
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.device == like.device and frames.dtype == torch.uint8
            and frames.is_contiguous() and frames.dim() == 3 and frames.shape[0] >= 1):
        raise ValueError(f"frames: expected a contiguous uint8 [n >= 1, H * 3 / 2, W] tensor on the GPU ({like.device}), got "
                         f"{(frames.dtype, frames.device, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames)}")
    return (frames.shape[0], *yuv_picture(frames.shape[1], frames.shape[2]))


def _surface_frames(frames, surface, like):
    """The check of frames read in place that the ``surface=`` forms of the frame wrappers share: ``surface`` a
    ``frames.Surface``; ``frames`` uint8 on the GPU of ``like``, either contiguous [n >= 1, ...] with
    ``surface.layout.frame_stride`` bytes per frame, or a strided view [n, H, W, C] of a packed format whose strides are that
    layout (``SurfaceLayout.of_view``).  Returns (n, H, W, the bytes from the first one the kernel may read)."""
    from .frames import Surface
    if not isinstance(surface, Surface):
        raise ValueError(f"surface: expected a frames.Surface, got {type(surface).__name__}")
    lay = surface.layout
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.device == like.device and frames.dtype == torch.uint8
            and frames.dim() >= 2 and frames.shape[0] >= 1):
        raise ValueError(f"frames: expected a uint8 [n >= 1, ...] tensor on the GPU ({like.device}), got "
                         f"{(frames.dtype, frames.device, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames)}")
    n = frames.shape[0]
    if frames.is_contiguous() and frames.numel() == n * lay.frame_stride:
        return n, lay.height, lay.width, frames.numel()
    if lay.fits_view(frames):
        return n, lay.height, lay.width, (n - 1) * lay.frame_stride + lay.extent
    raise ValueError(f"frames: shape {tuple(frames.shape)} with strides {tuple(frames.stride())} is neither contiguous with "
                     f"frame_stride = {lay.frame_stride} bytes per frame nor a view with the layout's strides")


def _yuv_entry(name, yuv, surface=None, nbytes=0):
    """The C entry ``name``, its ``_yuv`` sibling or its ``_surface`` sibling, and the arguments the sibling takes after
    ``frames``."""
    if surface is not None:
        if yuv is not None:
            raise ValueError("yuv and surface exclude each other: a surface carries its own conversion")
        return getattr(_lib.load(), name + "_surface"), (ctypes.c_size_t(nbytes), ctypes.byref(surface.desc()))
    return (getattr(_lib.load(), name), ()) if yuv is None else (getattr(_lib.load(), name + "_yuv"), (ctypes.byref(yuv),))


def _frames_in(frames, like, yuv, rows=None, surface=None):
    """The check of packed input frames that every frame wrapper shares: ``frames`` contiguous uint8 [n >= 1, H, W, 3] on
    the GPU of ``like`` (the ring or ``out``), 4:2:0 frames under ``yuv`` (``_yuv_frames``), or frames read in place under
    ``surface`` (``_surface_frames``); ``rows``: the n that ``out`` has room for.  Returns (n, H, W, the extent in bytes that
    only the surface entries ask for)."""
    nbytes = 0
    if surface is not None:
        n, h, w, nbytes = _surface_frames(frames, surface, like)
    elif yuv is not None:
        n, h, w = _yuv_frames(frames, yuv, like)
    elif not (torch.is_tensor(frames) and frames.is_cuda and frames.device == like.device and frames.dtype == torch.uint8
              and frames.is_contiguous() and frames.dim() == 4 and frames.shape[0] >= 1 and frames.shape[3] == 3):
        raise ValueError(f"frames: expected a contiguous uint8 [n >= 1, H, W, 3] tensor on the GPU of the ring or out ({like.device}), "
                         f"got {(frames.dtype, frames.device, tuple(frames.shape)) if torch.is_tensor(frames) else type(frames)}")
    else:
        n, h, w, _ = frames.shape
    if rows is not None and rows != n:
        raise ValueError(f"frames: {n} frames for the {rows} rows of out")
    return n, h, w, nbytes


def _clip_out(out, out_u8, crop_xyf, frames_per_group):
    """What only a clip call has: ``out`` contiguous float32 [n, 3, crop, crop] on the GPU; where asked for, ``out_u8`` uint8
    [n, crop, crop, 3] beside it; ``crop_xyf`` int32 [groups, 3], one entry per ``frames_per_group`` of the n frames.
    Returns (n, crop, frames_per_group)."""
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4
            and out.shape[1] == 3 and out.shape[2] == out.shape[3]):
        raise ValueError("out: expected a contiguous float32 [n, 3, crop, crop] GPU tensor")
    n, crop = out.shape[0], out.shape[2]
    if out_u8 is not None and not (torch.is_tensor(out_u8) and out_u8.is_cuda and out_u8.device == out.device and out_u8.dtype == torch.uint8
                                   and out_u8.is_contiguous() and tuple(out_u8.shape) == (n, crop, crop, 3)):
        raise ValueError(f"out_u8: expected a contiguous uint8 [{n}, {crop}, {crop}, 3] tensor on the GPU of out")
    g = int(frames_per_group)
    if g < 1:
        raise ValueError(f"frames_per_group = {g}: must be >= 1")
    _i32_table(crop_xyf, "crop_xyf", ((n + g - 1) // g, 3), out)
    return n, crop, g


def _resample_tables(tables, size, like):
    """``tables`` = (hbounds, hcoef, vbounds, vcoef) of ``frames.resample_tables`` as int32 [size, 2] / [size, k] GPU tensors."""
    hb, hk, vb, vk = tables
    for t, name, cols in ((hb, "hbounds", 2), (vb, "vbounds", 2), (hk, "hcoef", None), (vk, "vcoef", None)):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError(f"{name}: expected an int32 [size, k] GPU tensor")
        _i32_table(t, name, (int(size), cols if cols is not None else t.shape[1]), like)
    return hb, hk, vb, vk


def frames_stream_append(frames, tables, span, size, crop_xyf, row_stream, row_pos, max_count, u8ring, yuv=None, surface=None):
    """GroupScale(size) -> crop -> flip of the raw frames ``frames`` [n, H, W, 3] uint8 into the ring ``u8ring``
    [S, Rf, crop, crop, 3]: row m of the row table (``stream_row_table``) is frame m and lands in slot
    (row_stream[m], row_pos[m] % Rf).  ``tables``: (hbounds, hcoef, vbounds, vcoef) of ``frames.resample_tables`` for
    (W -> size, H -> size) as int32 GPU tensors; ``span``: the most input rows one band of output rows needs;
    ``crop_xyf`` int32 [S, 3]: (x1, y1, flip) per stream; ``max_count``: the most rows any one stream has in the table.
    The bytes are ``return_u8`` of ``FrameTransform`` for the same frame and crop entry.  ``yuv``: ``frames`` are 4:2:0
    frames [n, H * 3 / 2, W] (``_yuv_frames``), converted where the kernel reads them; the tables stay those of H and W.
    ``surface``: a ``frames.Surface`` -- ``frames`` are read in place in its layout's byte order, pitches and offsets
    (``_surface_frames``; a strided view is accepted), with the same result as the RGB call on the converted frames."""
    s, rf, crop = _u8_ring(u8ring)
    n, h, w, nbytes = _frames_in(frames, u8ring, yuv, None, surface)
    m = _row_table(row_stream, row_pos, u8ring)
    hb, hk, vb, vk = _resample_tables(tables, size, u8ring)
    _i32_table(crop_xyf, "crop_xyf", (s, 3), u8ring)
    entry, how = _yuv_entry("cer_frames_stream_append", yuv, surface, nbytes)
    check(entry(ptr(frames), *how, n, h, w, ptr(hb), ptr(hk), hk.shape[1], ptr(vb), ptr(vk), vk.shape[1], int(size), crop,
                ptr(crop_xyf), int(span), ptr(row_stream), ptr(row_pos), m, int(max_count), ptr(u8ring), s, rf, current_stream()),
          entry.__name__)
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("frames_append", 0))


def frames_transform(frames, tables, span, size, crop_xyf, frames_per_group, mean, std, out, out_u8=None, yuv=None, surface=None):
    """GroupScale(size) -> crop -> flip -> ToTensor -> Normalize of the raw frames ``frames`` [n, H, W, 3] uint8 into ``out``
    [n, 3, crop, crop] float32 (and ``out_u8`` [n, crop, crop, 3]), the clip form of ``frames_stream_append``: ``tables`` and
    ``span`` as there; ``crop_xyf`` int32 [groups, 3] on the GPU, one (x1, y1, flip) per ``frames_per_group`` frames.
    ``yuv``, ``surface``: as there."""
    n, crop, g = _clip_out(out, out_u8, crop_xyf, frames_per_group)
    _, h, w, nbytes = _frames_in(frames, out, yuv, n, surface)
    hb, hk, vb, vk = _resample_tables(tables, size, out)
    entry, how = _yuv_entry("cer_frames_transform", yuv, surface, nbytes)
    check(entry(ptr(frames), *how, n, h, w, ptr(hb), ptr(hk), hk.shape[1], ptr(vb), ptr(vk), vk.shape[1], int(size), crop,
                ptr(crop_xyf), g, int(span), float(mean), float(std), ptr(out), ptr(out_u8), current_stream()), entry.__name__)


# ------------------------------------------------------------------ per-frame tables: face boxes (csrc/frames_box.hip) and
# affine maps (csrc/frames_affine.hip).  ``geom`` is the ``frames.BoxTables`` / ``frames.AffineGeometry`` of the call: its
# ``stem`` names the C entries, ``check_rows`` vets the device table, ``entry_args`` gives its two device tables and three ints.
def stream_row_box_table(positions, counts, boxes, device):
    """``stream_row_table`` and the boxes of the same rows in ONE upload: ``boxes`` int [M, 4] on the host, row m the box of
    packed frame m -> (row_stream [M], row_pos [M], boxes [M, 4]), int32 views of one fresh tensor on ``device``."""
    row_stream, row_pos, words = _upload_rows(positions, counts, device, boxes, np.int32, 4, "stream_row_box_table")
    return row_stream, row_pos, words.view(-1, 4)


def stream_row_affine_table(positions, counts, affines, device):
    """``stream_row_table`` and the affines of the same rows in ONE upload: ``affines`` float64 [M, 6] on the host, row m the
    Pillow coefficients of packed frame m -> (row_stream [M], row_pos [M], affines [M, 6] float64), views of one fresh int32
    tensor on ``device``.  The doubles travel as int32 pairs at the head of the tensor, so they sit at its 8-byte aligned
    start whatever M."""
    row_stream, row_pos, words = _upload_rows(positions, counts, device, affines, np.float64, 6, "stream_row_affine_table")
    return row_stream, row_pos, words.view(torch.float64).view(-1, 6)


def _transform_rows(frames, rows, geom, size, crop_xyf, frames_per_group, mean, std, out, out_u8, yuv, surface):
    """The clip call of a per-frame table: ``frames_transform_boxes`` / ``frames_transform_affine``."""
    n, crop, g = _clip_out(out, out_u8, crop_xyf, frames_per_group)
    _, h, w, nbytes = _frames_in(frames, out, yuv, n, surface)
    geom.check_rows(rows, n, size, crop, out)
    a, b, *ints = geom.entry_args(out.device)
    entry, how = _yuv_entry("cer_frames_transform_" + geom.stem, yuv, surface, nbytes)
    check(entry(ptr(frames), *how, n, h, w, ptr(rows), ptr(a), ptr(b), *ints, int(size), crop, ptr(crop_xyf), g, float(mean),
                float(std), ptr(out), ptr(out_u8), current_stream()), entry.__name__)


def _append_rows(frames, rows, geom, size, crop_xyf, row_stream, row_pos, max_count, u8ring, yuv, surface):
    """The ring call of a per-frame table: ``frames_stream_append_boxes`` / ``frames_stream_append_affine``."""
    s, rf, crop = _u8_ring(u8ring)
    n, h, w, nbytes = _frames_in(frames, u8ring, yuv, None, surface)
    m = _row_table(row_stream, row_pos, u8ring)
    geom.check_rows(rows, m, size, crop, u8ring)
    _i32_table(crop_xyf, "crop_xyf", (s, 3), u8ring)
    a, b, *ints = geom.entry_args(u8ring.device)
    entry, how = _yuv_entry("cer_frames_stream_append_" + geom.stem, yuv, surface, nbytes)
    check(entry(ptr(frames), *how, n, h, w, ptr(rows), ptr(a), ptr(b), *ints, int(size), crop, ptr(crop_xyf), ptr(row_stream),
                ptr(row_pos), m, int(max_count), ptr(u8ring), s, rf, current_stream()), entry.__name__)
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("frames_append_" + geom.stem, 0))


def frames_transform_boxes(frames, boxes, store, size, crop_xyf, frames_per_group, mean, std, out, out_u8=None, yuv=None, surface=None):
    """``Image.crop(boxes[f])`` -> GroupScale(size) -> crop -> flip -> ToTensor -> Normalize of full frames ``frames``
    [n, H, W, 3] uint8 into ``out`` [n, 3, crop, crop] float32 (and ``out_u8`` [n, crop, crop, 3]).  ``boxes`` int32 [n, 4]
    on the GPU = (x0, y0, x1, y1), right and lower exclusive, zero outside the frame; the kernel clamps what it is given
    (coordinates into +-2^20, sides into 1 .. ``store.max_side``), so a table nobody vetted gives wrong numbers and no
    access outside ``frames``.  ``store``: ``frames.box_tables(size, max_side)``; ``crop_xyf`` int32 [groups, 3] on the GPU,
    one entry per ``frames_per_group`` frames.  ``yuv``: ``frames`` are 4:2:0 frames [n, H * 3 / 2, W] (``_yuv_frames``); the
    boxes stay in luma pixels and what lies outside the picture is RGB 0.  ``surface``: as in ``frames_stream_append``."""
    _transform_rows(frames, boxes, store, size, crop_xyf, frames_per_group, mean, std, out, out_u8, yuv, surface)


def frames_stream_append_boxes(frames, boxes, store, size, crop_xyf, row_stream, row_pos, max_count, u8ring, yuv=None, surface=None):
    """``frames_stream_append`` of full frames with one box per row: row m of the row table is packed frame m, cropped to
    ``boxes[m]`` as ``frames_transform_boxes`` does, and lands in slot (row_stream[m], row_pos[m] % Rf).  The bytes are
    ``return_u8`` of ``FrameTransform(..., boxes=)`` for the same frame, box and crop entry.  ``yuv``, ``surface``: as there."""
    _append_rows(frames, boxes, store, size, crop_xyf, row_stream, row_pos, max_count, u8ring, yuv, surface)


def frames_transform_affine(frames, affines, geom, size, crop_xyf, frames_per_group, mean, std, out, out_u8=None, yuv=None, surface=None):
    """``Image.transform((A, A), AFFINE, affines[f], BILINEAR)`` -> GroupScale(size) -> crop -> flip -> ToTensor -> Normalize
    of full frames ``frames`` [n, H, W, 3] uint8 into ``out`` [n, 3, crop, crop] float32 (and ``out_u8`` [n, crop, crop, 3]).
    ``affines`` float64 [n, 6] on the GPU, Pillow's coefficients (output pixel centre -> frame coordinate); the kernel only
    compares and multiplies them and fetches every pixel at a clamped index, so a table nobody vetted -- NaN, infinities,
    1e300 -- gives the all-zero picture and no access outside ``frames``.  ``geom``: ``frames.affine_geometry(A, size)``;
    ``crop_xyf`` int32 [groups, 3] on the GPU, one entry per ``frames_per_group`` frames.  ``yuv``: ``frames`` are 4:2:0
    frames [n, H * 3 / 2, W] (``_yuv_frames``); the four pixels of a sample are converted, then interpolated.  ``surface``: as
    in ``frames_stream_append``."""
    _transform_rows(frames, affines, geom, size, crop_xyf, frames_per_group, mean, std, out, out_u8, yuv, surface)


def frames_stream_append_affine(frames, affines, geom, size, crop_xyf, row_stream, row_pos, max_count, u8ring, yuv=None, surface=None):
    """``frames_stream_append`` of full frames with one affine per row: row m of the row table is packed frame m, warped by
    ``affines[m]`` as ``frames_transform_affine`` does, and lands in slot (row_stream[m], row_pos[m] % Rf).  The bytes are
    ``return_u8`` of ``FrameTransform.aligned`` for the same frame, affine and crop entry.  ``yuv``, ``surface``: as there."""
    _append_rows(frames, affines, geom, size, crop_xyf, row_stream, row_pos, max_count, u8ring, yuv, surface)


def frames_stream_gather(u8ring, row_stream, row_pos, mean=0.5, std=0.5):
    """out[m] = ((u8ring[row_stream[m], row_pos[m] % Rf] / 255) - mean) / std as float32 [M, 3, crop, crop]: the tensor
    ``FrameTransform`` gives the same frames."""
    s, rf, crop = _u8_ring(u8ring)
    m = _row_table(row_stream, row_pos, u8ring)
    out = torch.empty((m, 3, crop, crop), device=u8ring.device, dtype=torch.float32)
    check(_lib.load().cer_frames_stream_gather(ptr(u8ring), s, rf, crop, ptr(row_stream), ptr(row_pos), m, float(mean), float(std),
                                               ptr(out), current_stream()), "cer_frames_stream_gather")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("frames_gather", 0))
    return out


# ------------------------------------------------------------------ running decisions (csrc/decision_stream.hip)
DECISION_NEVER = (1 << 63) - 1   # ``first`` of a class no frame has been predicted as


def decision_stream_state(streams, n_out, *, window=None, max_new=32, classify=True, device="cuda"):
    """The device state of ``streams`` reset streams as a dict.  Whole-stream (``window`` None): ``slog`` [S, C] float64 and,
    with ``classify``, ``votes`` / ``first`` [S, C] int64 and ``sprob`` [S, C] float64.  Window: ``zring`` [S, R, C] float32, R
    the power of two >= window + max_new."""
    if window is None:
        state = {"slog": torch.zeros((streams, n_out), dtype=torch.float64, device=device)}
        if classify:
            state["votes"] = torch.zeros((streams, n_out), dtype=torch.int64, device=device)
            state["first"] = torch.full((streams, n_out), DECISION_NEVER, dtype=torch.int64, device=device)
            state["sprob"] = torch.zeros((streams, n_out), dtype=torch.float64, device=device)
        return state
    r = pow2_at_least(int(window) + int(max_new))
    return {"zring": torch.zeros((streams, r, n_out), dtype=torch.float32, device=device)}


def _decision_state(state, window, classify):
    """Check the state tensors of the mode.  Returns (descriptor without M / max_count, the five pointers, device)."""
    def want(name, dtype, shape=None):
        t = state.get(name)
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
                and (shape is None or tuple(t.shape) == tuple(shape))):
            raise ValueError(f"{name}: expected a contiguous {dtype} GPU tensor" + (f" of shape {tuple(shape)}" if shape else "")
                             + f", got {(t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t)}")
        return t
    d = _lib.DecisionStreamDesc(classify=int(bool(classify)))
    if window is None:
        slog = want("slog", torch.float64)
        if slog.dim() != 2:
            raise ValueError(f"slog: expected [S, C], got {tuple(slog.shape)}")
        d.S, d.C = slog.shape
        names = ("votes", "first", "sprob") if classify else ()
        ts = {n: want(n, torch.float64 if n == "sprob" else torch.int64, slog.shape) for n in names}
        if any(t.device != slog.device for t in ts.values()):
            raise ValueError("the state tensors sit on different devices")
        return d, (_addr(ts.get("votes")), _addr(ts.get("first")), _addr(slog), _addr(ts.get("sprob")), None), slog.device
    window = int(window)
    if window < 1:
        raise ValueError(f"window = {window}: must be >= 1, or None for the whole stream")
    d.S, d.R, d.C = _ring(want("zring", torch.float32), "zring")
    d.W = window
    return d, (None, None, None, None, _addr(state["zring"])), state["zring"].device


def decision_stream_push(rows, segments, max_count, state, *, window=None, drop_last=False, classify=True, track=False):
    """Append the packed rows ``rows`` [M, C] of one push to the streams' state as the table ``segments``
    (``decision_segment_table``) says; ``max_count``: the largest count in it.  ``track``: also return (decisions [M, 3] int32
    or None without ``classify``, means [M, 2, C]) as they stand after each new row."""
    d, state_ptrs, dev = _decision_state(state, window, classify)
    _dev_f32(rows, "rows")
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] != d.C or rows.shape[0] < 1 or rows.device != dev:
        raise ValueError(f"rows: expected [M >= 1, {d.C}] on {dev}, got "
                         f"{(tuple(rows.shape), rows.device) if torch.is_tensor(rows) else type(rows)}")
    a = _stream_table(segments, "segments", DECISION_FIELDS, rows)
    d.M, d.max_count, d.drop_last = rows.shape[0], int(max_count), int(bool(drop_last))
    dec = torch.empty((d.M, 3), dtype=torch.int32, device=dev) if track and classify else None
    means = torch.empty((d.M, 2, d.C), dtype=torch.float32, device=dev) if track else None
    check(_lib.load().cer_decision_stream_push(ctypes.byref(d), rows.data_ptr(), segments.data_ptr(), a, *state_ptrs, _addr(dec),
                                               _addr(means), current_stream()), "cer_decision_stream_push")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("decision_push", 0))
    return (dec, means) if track else None


def decision_stream_read(table, max_count, state, *, window=None, drop_last=False, classify=True):
    """The decisions as they stand: ``table`` [6, S] (``decision_segment_table``, one entry per stream in stream order: count
    = rows in the window, position = where the next row goes, frames since reset) -> (decisions [S, 3] int32 with -1 for a
    stream without a frame, or None without ``classify``; means [S, 2, C], NaN for such a stream)."""
    d, state_ptrs, dev = _decision_state(state, window, classify)
    like = state["slog"] if window is None else state["zring"]
    if _stream_table(table, "table", DECISION_FIELDS, like) != d.S:
        raise ValueError(f"table: expected one entry per stream ({d.S}), got {table.shape[1]}")
    d.M, d.max_count, d.drop_last = 1, int(max_count), int(bool(drop_last))
    dec = torch.empty((d.S, 3), dtype=torch.int32, device=dev) if classify else None
    means = torch.empty((d.S, 2, d.C), dtype=torch.float32, device=dev)
    check(_lib.load().cer_decision_stream_read(ctypes.byref(d), table.data_ptr(), *state_ptrs, _addr(dec), means.data_ptr(),
                                               current_stream()), "cer_decision_stream_read")
    if STREAM_TRACE is not None:
        STREAM_TRACE.append(("decision_read", 0))
    return dec, means
