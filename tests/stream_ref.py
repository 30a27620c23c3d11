"""References and case tables of the streaming TCN tests (``tests/test_stream_cpu.py``, ``tests/test_stream_gpu.py``).

Nothing here needs a GPU.

* ``block_ref``: one ``TemporalBlock`` over a WHOLE sequence in float64, built from ``conv_ref.conv_ref`` on the geometry of
  ``conv_ref.causal_case``.  By causality it is the reference of any frame-at-a-time evaluation.

* EXACT cases follow the convention of ``tests/conv_ref.py``: integer x in [-2, 2], w in {-1, 0, 1}, integer biases,
  slope 0.25.  Then every value of a block is a multiple of a dyadic unit:

      pre-activation 1 (conv1 + b1), the projection of the residual                 units of 1
      h = leaky(pre 1), pre-activation 2 (conv2(h) + b2)                           units of 1/4
      inner = leaky(pre 2), inner + res                                            units of 1/16
      out = leaky(inner + res)                                                     units of 1/64

  ``exact_margins`` scales each to its unit; the CPU test asserts all below 2^24.  It also bounds the partial sums of ANY
  order through the magnitude twins (the same convs on |x|, |w|: the sum of |products| of one output, plus |bias|), so every
  fp32 operation of the kernel is exact whatever its reduction order and the streamed result must equal ``block_ref`` BIT FOR
  BIT.  One block is the largest such unit: a second block's magnitudes pass 2^24, so stacks are tested with normal data.

* ``ring_emulation``: the semantics of the two C entry points restated in float64 torch on the CPU (append; conv with the taps
  gathered from a ring), so that the ring algebra itself -- slots, heads, wraps, chunking -- is checked without a GPU.
"""
from collections import namedtuple

import torch

import conv_ref

SLOPE = conv_ref.SLOPE
LIMIT = 2.0 ** 24

# cin cout: channels.  k dil: the convs.  ds: 1x1 projection of the residual (else identity: cin == cout).  s: streams.
# max_new: the largest push (fixes R).  mixed: chunk sizes 1, 3, 2, max_new, 1, ... clipped to max_new (else all 1).
# misalign: floats the rings are shifted off a 16-byte boundary (0: the float4 path, else the element-wise one).
BlockCase = namedtuple("BlockCase", "name cin cout k dil ds s max_new mixed misalign")


def _bc(cin, cout, k, dil, ds, s, max_new, mixed, misalign=0):
    name = f"{cin}to{cout}_k{k}_d{dil}_{'ds' if ds else 'id'}_S{s}_new{max_new}_{'mixed' if mixed else 'ones'}_off{misalign}"
    return BlockCase(name, cin, cout, k, dil, ds, s, max_new, mixed, misalign)


# (Cin, Cout) in {(5, 3), (39, 32), (128, 32), (32, 130)} with the projection (Cin != Cout needs it); the identity residual on
# (Cout, Cout) of the same sizes; every k in {1, 2, 5}, d in {1, 8}, S in {1, 3, 33}, max_new in {1, 3}, both chunkings.
# k = 1 with max_new = 1 is the one-slot ring (R = 1).  Cout = 3 / 130: a ragged last tile of 4 channels; S * c = 1 .. 99 rows:
# one ragged tile of 8 rows up to 13 tiles.
BLOCK_CASES = [
    _bc(5, 3, 5, 1, True, 1, 1, False),
    _bc(5, 3, 2, 8, True, 33, 3, True),
    _bc(39, 32, 5, 8, True, 3, 3, True),
    _bc(39, 32, 1, 1, True, 33, 1, False),
    _bc(128, 32, 5, 8, True, 1, 3, False),
    _bc(128, 32, 2, 1, True, 3, 3, True, misalign=1),
    _bc(32, 130, 5, 1, True, 3, 1, False),
    _bc(32, 130, 1, 8, True, 1, 3, True),
    _bc(3, 3, 5, 8, False, 3, 3, True),
    _bc(32, 32, 5, 1, False, 33, 3, True),
    _bc(32, 32, 5, 8, False, 3, 3, True, misalign=3),
    _bc(130, 130, 2, 8, False, 1, 1, False),
    _bc(32, 32, 1, 1, False, 1, 3, False),
]


def ring_frames(k, dil, max_new):
    need, r = (k - 1) * dil + max_new, 1
    while r < need:
        r *= 2
    return r


def frames_of(case):
    """T >= 3 R: every ring wraps at least twice."""
    return 3 * ring_frames(case.k, case.dil, case.max_new) + 2


def chunks_of(case, total):
    """The push sizes of a case, summing to ``total``."""
    pattern = [min(c, case.max_new) for c in (1, 3, 2, case.max_new)] if case.mixed else [1]
    out, i = [], 0
    while sum(out) < total:
        out.append(min(pattern[i % len(pattern)], total - sum(out)))
        i += 1
    return out


def _seed(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode())) % (2 ** 31)


def make_block(case):
    """float32 CPU operands of an exact case: x [S, T, Cin], w1 [Cout, Cin, k], b1, w2 [Cout, Cout, k], b2, dsw [Cout, Cin, 1]
    or None, dsb or None."""
    g = torch.Generator().manual_seed(_seed(case.name))
    ints = (lambda shape, lim: torch.randint(-lim, lim + 1, shape, generator=g).float())
    d = {"x": ints((case.s, frames_of(case), case.cin), 2),
         "w1": ints((case.cout, case.cin, case.k), 1), "b1": ints((case.cout,), 4),
         "w2": ints((case.cout, case.cout, case.k), 1), "b2": ints((case.cout,), 4),
         "dsw": None, "dsb": None}
    if case.ds:
        d["dsw"], d["dsb"] = ints((case.cout, case.cin, 1), 1), ints((case.cout,), 4)
    else:
        assert case.cin == case.cout
    return d


def _causal(x_stc, w_oik, k, dil, **kw):
    """``conv_ref`` on the causal geometry of ``conv_ref.causal_case``: x [S, T, C] -> (y, aux, raw), each [S, T, Cout]."""
    s, t, _ = x_stc.shape
    y, aux, raw = conv_ref.conv_ref(x_stc.reshape(s, t, 1, -1), w_oik.unsqueeze(-1), dil=(dil, 1), pad_t=(k - 1) * dil,
                                    out_hw=(t, 1), **kw)
    return y.reshape(s, t, -1), aux.reshape(s, t, -1), raw.reshape(s, t, -1)


def block_ref(x, w1, b1, w2, b2, dsw, dsb, k, dil, slope=SLOPE):
    """One TemporalBlock (eval) over the whole sequence x [S, T, Cin], float64.  Returns every intermediate."""
    x = x.double()
    h, _, raw1 = _causal(x, w1, k, dil, bias=b1, act1=conv_ref.ACT_LEAKY, slope=slope)
    res = x if dsw is None else _causal(x, dsw, 1, 1, bias=dsb)[0]
    out, inner, raw2 = _causal(h, w2, k, dil, bias=b2, act1=conv_ref.ACT_LEAKY, slope=slope,
                               residual=res.reshape(*res.shape[:2], 1, -1), act2=conv_ref.ACT_LEAKY)
    return {"pre1": raw1 + b1.double(), "h": h, "pre2": raw2 + b2.double(), "inner": inner, "res": res, "sum": inner + res,
            "out": out}


def exact_margins(case, d):
    """name -> max |value| / unit over an exact case: the intermediates of the block and the magnitude twins that bound the
    partial sums of any reduction order.  All must stay below 2^24."""
    r = block_ref(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["dsw"], d["dsb"], case.k, case.dil)
    m = {"pre1": r["pre1"].abs().max().item(), "h": r["h"].abs().max().item() * 4, "pre2": r["pre2"].abs().max().item() * 4,
         "inner": r["inner"].abs().max().item() * 16, "sum": r["sum"].abs().max().item() * 16,
         "out": r["out"].abs().max().item() * 64}
    for name, v in r.items():   # each IS a multiple of its unit
        unit = {"pre1": 1, "res": 1, "h": 4, "pre2": 4, "inner": 16, "sum": 16, "out": 64}[name]
        assert torch.equal(v * unit, (v * unit).round()), name
    mag1 = _causal(d["x"].double().abs(), d["w1"].abs(), case.k, case.dil)[2] + d["b1"].double().abs()
    mag2 = _causal(r["h"].abs(), d["w2"].abs(), case.k, case.dil)[2] + d["b2"].double().abs()
    m["mag1"], m["mag2"] = mag1.max().item(), mag2.max().item() * 4
    magres = r["res"].abs()
    if d["dsw"] is not None:
        magres = _causal(d["x"].double().abs(), d["dsw"].abs(), 1, 1)[2] + d["dsb"].double().abs()
        m["magres"] = magres.max().item()
    m["magsum"] = (mag2 + magres).max().item() * 64      # |inner| + |res| bounds the sum and the output, in units of 1/64
    return m


# ---------------------------------------------------------------------------------------------- the entry points, restated
class ring_emulation:
    """``ops.tcn_stream_append`` / ``ops.tcn_stream_conv`` on CPU tensors of any float dtype, weights UNPACKED ([Cout, Cin, k];
    ``res_w`` [Cout, Cin, 1]).  Same argument names as the wrappers."""

    @staticmethod
    def append(rows, ring, head):
        r = ring.shape[1]
        for i in range(rows.shape[1]):
            ring[:, (head + i) & (r - 1)] = rows[:, i]

    @staticmethod
    def conv(ring, head, c, w, bias, k, dil, *, res_ring=None, res_head=0, res_w=None, res_bias=None, out_ring=None, out_head=0,
             out_dense=None, slope=SLOPE):
        s, r, _ = ring.shape
        assert r & (r - 1) == 0 and 0 <= head < r and 1 <= c <= r - (k - 1) * dil
        leaky = (lambda v: torch.where(v >= 0, v, v * slope))
        for i in range(c):
            z = bias.clone().expand(s, -1).clone()
            for j in range(k):
                z += ring[:, (head + i - (k - 1 - j) * dil) & (r - 1)] @ w[:, :, j].T
            v = leaky(z)
            if res_ring is not None:
                res = res_ring[:, (res_head + i) & (res_ring.shape[1] - 1)]
                if res_w is not None:
                    res = res @ res_w[:, :, 0].T + res_bias
                v = leaky(v + res)
            if out_ring is not None:
                out_ring[:, (out_head + i) & (out_ring.shape[1] - 1)] = v
            if out_dense is not None:
                out_dense.view(s, c, -1)[:, i] = v


def stream_block_emulated(case, d, dtype=torch.float64):
    """An exact case pushed through the emulated entry points with the case's chunking: out [S, T, Cout]."""
    r = ring_frames(case.k, case.dil, case.max_new)
    cv = (lambda t: None if t is None else t.to(dtype))
    x, w1, b1, w2, b2, dsw, dsb = (cv(d[n]) for n in ("x", "w1", "b1", "w2", "b2", "dsw", "dsb"))
    xring, hring = torch.zeros(case.s, r, case.cin, dtype=dtype), torch.zeros(case.s, r, case.cout, dtype=dtype)
    outs, pos = [], 0
    for c in chunks_of(case, x.shape[1]):
        head = pos & (r - 1)
        ring_emulation.append(x[:, pos:pos + c], xring, head)
        ring_emulation.conv(xring, head, c, w1, b1, case.k, case.dil, out_ring=hring, out_head=head)
        dense = torch.empty(case.s * c, case.cout, dtype=dtype)
        ring_emulation.conv(hring, head, c, w2, b2, case.k, case.dil, res_ring=xring, res_head=head, res_w=dsw, res_bias=dsb,
                            out_dense=dense)
        outs.append(dense.view(case.s, c, -1))
        pos += c
    return torch.cat(outs, dim=1)
