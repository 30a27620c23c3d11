"""The attention kernels (csrc/attention.hip: forward, dQ, dK/dV, each plain and SPLIT, d = 32 / 64 / 128) against the
float64 reference of tests/attention_ref.py, at the inputs where such kernels go wrong: whole key tiles masked, rows with
no visible key, ragged ends, the split threshold, BERT's and the cross-attention's memory layouts, scores of magnitude
100, and twice in a row for bit-identical results.  The case tables live in attention_ref.py and are checked without a
GPU by test_attention_cases_cpu.py (which kernels each case reaches, what each mask masks).

Every case runs in guarded buffers: q / k / v / dout sit in NaN-filled allocations (a read past a ragged end poisons the
result), out / dq / dk / dv / lse in sentinel-filled ones with a guard row before and after every batch row and four guard
columns after every head; the guards must come back untouched and every element inside must have been written.

Bars.  Standard-normal inputs keep the project's bars, now against float64: 2e-5 on out, 5e-5 on the gradients, and lse at
1e-5 relative (|lse| < 1 counted as 1: lse crosses zero).  Extreme inputs have no fixed bar: the yardstick is the SAME
reference evaluated in float32 by torch on the CPU (max-subtracted softmax, the kernel's formulas in another summation
order), its error against float64 floored at one fp32 rounding of the largest reference element (2^-24 max|ref|: no fp32
result is expected to be closer), and the kernel is allowed 4 x that -- the factor covers a different summation order
over up to 1024 keys and the forward pre-scaling Q while the backward scales the product.
"""
import math

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
OUTPUTS = ("out", "dq", "dk", "dv")
BAR_OUT, BAR_GRAD, BAR_LSE_REL, YARD_FACTOR = 2e-5, 5e-5, 1e-5, 4.0


# ---------------------------------------------------------------------------------------------- guarded runs
def padded_layout(b, h, sq, sk, d):
    """Every tensor in a buffer of its own: [B, S + 2, H, d + 4], the tensor at rows 1 .. S and columns 0 .. d - 1."""
    def slot(name, s):
        return (name, (b, s + 2, h, d + 4), lambda t: t[:, 1:s + 1, :, :d])
    return {n: slot(n, s) for n, s in (("q", sq), ("k", sk), ("v", sk), ("out", sq), ("dout", sq), ("dq", sq), ("dk", sk),
                                       ("dv", sk))}


def bert_layout(b, s, h, d):
    """BertEncoderHIP's layout: Q, K, V as column blocks of one [B*S, 3*hidden] buffer (head stride d), out in [B, S, hidden];
    dout a column block of a wider buffer (other strides than out), dq / dk / dv column blocks of one buffer.  One guard row
    before the first token and one after the last."""
    hid, n = h * d, b * s

    def fused(i):
        return lambda t: t[1:1 + n].view(b, s, 3, h, d)[:, :, i]
    lay = {nm: ("qkv", (n + 2, 3 * hid), fused(i)) for i, nm in enumerate(("q", "k", "v"))}
    lay.update({nm: ("dqkv", (n + 2, 3 * hid), fused(i)) for i, nm in enumerate(("dq", "dk", "dv"))})
    lay["out"] = ("out", (n + 2, hid), lambda t: t[1:1 + n].view(b, s, h, d))
    lay["dout"] = ("dout", (n + 2, 2 * hid), lambda t: t[1:1 + n, hid:].unflatten(0, (b, s)).unflatten(2, (h, d)))
    return lay


def cross_layout(b, sq, sk, e):
    """fusion_heads.py's cross-attention: Q rows [B*Sq, E], K and V the two column blocks of one [B*Sk, 2E] buffer, one head;
    dq in a buffer of its own, dk / dv the column blocks of one [B*Sk, 2E] buffer."""
    def rows(s, lo, hi):
        return lambda t: t[1:1 + b * s, lo:hi].unflatten(0, (b, s)).unsqueeze(2)
    return {"q": ("q", (b * sq + 2, e), rows(sq, 0, e)), "k": ("kv", (b * sk + 2, 2 * e), rows(sk, 0, e)),
            "v": ("kv", (b * sk + 2, 2 * e), rows(sk, e, 2 * e)), "out": ("out", (b * sq + 2, e), rows(sq, 0, e)),
            "dout": ("dout", (b * sq + 2, e + 4), rows(sq, 4, e + 4)), "dq": ("dq", (b * sq + 2, e), rows(sq, 0, e)),
            "dk": ("dkv", (b * sk + 2, 2 * e), rows(sk, 0, e)), "dv": ("dkv", (b * sk + 2, 2 * e), rows(sk, e, 2 * e))}


def run_kernels(q, k, v, dout, mask, scale, layout=None):
    """Forward + backward in guarded buffers.  Returns the CPU results {"out", "lse", "dq", "dk", "dv"} after asserting
    that nothing outside the tensors was written and everything inside was."""
    from feature_vs_text_compound_emotion_amd import ops
    b, sq, h, d = q.shape
    sk = k.shape[1]
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    layout = layout or padded_layout(b, h, sq, sk, d)
    bufs, is_out = {}, {}
    for name, (key, shape, _) in layout.items():
        out = name in OUTPUTS
        assert is_out.setdefault(key, out) == out, "a buffer holds inputs or outputs, not both"
        if key not in bufs:
            bufs[key] = torch.full(shape, SENTINEL if out else float("nan"), device="cuda", dtype=torch.float32)
    view = {name: fn(bufs[key]) for name, (key, _, fn) in layout.items()}
    for name, t in (("q", q), ("k", k), ("v", v), ("dout", dout)):
        assert tuple(view[name].shape) == tuple(t.shape) and view[name].stride(3) == 1, name
        view[name].copy_(t.cuda())
    n_lse = b * h * sq
    lse_buf = torch.full((n_lse + 128,), SENTINEL, device="cuda", dtype=torch.float32)
    lse = lse_buf[64:64 + n_lse].view(b, h, sq)
    dmask = None if mask is None else mask.to(torch.int32).cuda().contiguous()

    def st(name):
        assert view[name].stride(3) == 1
        return tuple(view[name].stride()[:3])
    ops.attention(view["q"], view["k"], view["v"], view["out"], b, h, sq, sk, d, st("q"), st("k"), st("v"), st("out"), scale,
                  key_mask=dmask, lse=lse)
    ops.attention_bwd(view["q"], view["k"], view["v"], view["out"], view["dout"], lse, view["dq"], view["dk"], view["dv"],
                      b, h, sq, sk, d, st("q"), st("k"), st("v"), st("out"), st("dout"), st("dq"), st("dk"), st("dv"), scale,
                      key_mask=dmask)
    torch.cuda.synchronize()
    for key, buf in bufs.items():
        if not is_out[key]:
            continue
        inside = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
        for name, (k2, _, fn) in layout.items():
            if k2 == key:
                fn(inside).fill_(True)
        assert bool((buf[~inside] == SENTINEL).all()), f"{key}: a guard row or column was written"
        assert not bool((buf[inside] == SENTINEL).any()), f"{key}: an element inside the tensor was never written"
    assert bool((lse_buf[:64] == SENTINEL).all()) and bool((lse_buf[64 + n_lse:] == SENTINEL).all()), "lse guards written"
    assert not bool((lse == SENTINEL).any()), "an lse row was never written"
    res = {name: view[name].detach().cpu().clone() for name in OUTPUTS}
    res["lse"] = lse.cpu().clone()
    return res


def errors(got, ref):
    """Max abs error of out / dq / dk / dv, and of lse over the rows with a visible key (relative, |lse| < 1 counted as 1);
    rows without one must hold +inf exactly."""
    err = {n: (got[n].double() - ref[n].double()).abs().max().item() for n in OUTPUTS}
    live = torch.isfinite(ref["lse"])
    assert bool((got["lse"][~live] == float("inf")).all()), "a row with no visible key must have lse = +inf"
    lg, lr = got["lse"][live].double(), ref["lse"][live].double()
    err["lse_rel"] = ((lg - lr).abs() / lr.abs().clamp_min(1.0)).max().item() if lr.numel() else 0.0
    err["lse"] = (lg - lr).abs().max().item() if lr.numel() else 0.0
    return err


def assert_finite(got):
    for n in OUTPUTS:
        assert bool(torch.isfinite(got[n]).all()), f"{n} is not finite"
    assert not bool(torch.isnan(got["lse"]).any()), "lse holds a NaN"


def assert_standard_bars(got, ref, what):
    assert_finite(got)
    e = errors(got, ref)
    print(f"\n[attention {what}] out {e['out']:.2e} dq {e['dq']:.2e} dk {e['dk']:.2e} dv {e['dv']:.2e} "
          f"lse(rel) {e['lse_rel']:.2e}")
    assert e["out"] < BAR_OUT, (what, e)
    assert e["dq"] < BAR_GRAD and e["dk"] < BAR_GRAD and e["dv"] < BAR_GRAD, (what, e)
    assert e["lse_rel"] < BAR_LSE_REL, (what, e)


def assert_contract_on_dead_rows(got, mask):
    """Batch rows whose mask is all zero: out = 0, dq = 0, dk = dv = 0, lse = +inf; masked keys of any row: dk = dv = 0."""
    if mask is None:
        return
    dead = ~(mask != 0).any(-1)
    for n in OUTPUTS:
        assert bool((got[n][dead] == 0).all()), f"{n} of a batch row with no visible key must be zero"
    assert bool((got["lse"][dead] == float("inf")).all())
    gone = mask == 0
    assert bool((got["dk"][gone] == 0).all()) and bool((got["dv"][gone] == 0).all()), "a masked key got a gradient"


def _case(name, b, h, sq, sk, d, kind, scale, spec):
    q, k, v, dout = ar.make_inputs(name, b, h, sq, sk, d, kind)
    mask = ar.build_mask(spec, b, sk, ar.case_seed(name))
    return q, k, v, dout, mask


# ---------------------------------------------------------------------------------------------- masks and shapes
@pytest.mark.parametrize("case", ar.MASK_CASES, ids=[c[0] for c in ar.MASK_CASES])
def test_structured_masks(case):
    """Trailing padding of 1 / 31 / 32 / 33 / 64 / Sk keys, the first one or two tiles masked, one wave of the split
    variants seeing nothing, and one batch row with no visible key next to ordinary ones -- plain and split, every d."""
    name, b, h, sq, sk, d, spec = case
    q, k, v, dout, mask = _case(name, b, h, sq, sk, d, "randn", None, spec)
    got = run_kernels(q, k, v, dout, mask, None)
    assert_standard_bars(got, ar.attention_ref(q, k, v, mask, None, dout), name)
    assert_contract_on_dead_rows(got, mask)
    if spec[0] == "dead_row":
        # the neighbours are bit for bit what they are when that row attends every key
        alive = mask.clone()
        alive[spec[1]] = 1
        other = run_kernels(q, k, v, dout, alive, None)
        keep = [i for i in range(b) if i != spec[1]]
        for n in OUTPUTS + ("lse",):
            assert torch.equal(got[n][keep], other[n][keep]), f"{n}: a neighbour of the masked row changed"


@pytest.mark.parametrize("case", ar.SHAPE_CASES, ids=[c[0] for c in ar.SHAPE_CASES])
def test_shape_edges(case):
    """Sq = 1, Sk = 1, Sk = 33, Sq one past a multiple of 128 and of 32, Sk = 128 / 127 (the split threshold), shapes where
    only the forward / dQ or only dK/dV split, and long streams -- with and without a mask."""
    name, b, h, sq, sk, d, spec = case
    q, k, v, dout, mask = _case(name, b, h, sq, sk, d, "randn", None, spec)
    got = run_kernels(q, k, v, dout, mask, None)
    assert_standard_bars(got, ar.attention_ref(q, k, v, mask, None, dout), name)
    assert_contract_on_dead_rows(got, mask)


# ---------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("s", [80, 160])
def test_bert_fused_qkv_layout(s):
    """[B*S, 3*768] with 12 heads of 64, key padding to 5 / 33 / S tokens, out in [B, S, 768], dout with other strides than
    out, dq / dk / dv into the column blocks of one buffer.  S = 80 runs the plain kernels, S = 160 the split ones; with
    H = 12 the lse index (b * H + h) * Sq + q is exercised beyond H = 1."""
    b, h, d = 3, 12, 64
    assert ar.variants(b, h, s, s, d) == {(p, "split" if s >= 128 else "plain", d) for p in ("fwd", "dq", "dkv")}
    q, k, v, dout = ar.make_inputs(f"bert{s}", b, h, s, s, d)
    mask = torch.zeros(b, s, dtype=torch.int32)
    for i, n in enumerate((5, 33, s)):
        mask[i, :n] = 1
    got = run_kernels(q, k, v, dout, mask, None, bert_layout(b, s, h, d))
    assert_standard_bars(got, ar.attention_ref(q, k, v, mask, None, dout), f"bert-fused S={s}")
    assert_contract_on_dead_rows(got, mask)


@pytest.mark.parametrize("sq,sk", [(50, 140), (140, 50), (130, 130)])
def test_cross_attention_kv_buffer_layout(sq, sk):
    """K and V from one [Rk, 2E] buffer, dk / dv into one, dout offset by four columns in a wider buffer (E = 128, 1 head)."""
    b, e = 2, 128
    q, k, v, dout = ar.make_inputs(f"cross{sq}x{sk}", b, 1, sq, sk, e)
    got = run_kernels(q, k, v, dout, None, None, cross_layout(b, sq, sk, e))
    assert_standard_bars(got, ar.attention_ref(q, k, v, None, None, dout), f"cross {sq}x{sk}")


# ---------------------------------------------------------------------------------------------- extreme scores
@pytest.mark.parametrize("case", ar.EXTREME_CASES, ids=[c[0] for c in ar.EXTREME_CASES])
def test_extreme_scores_against_the_fp32_yardstick(case):
    """Q and K times 5 (|score| up to ~100-150: an unshifted expf overflows), a scale that is not 1 / sqrt(d) (1.0 at
    d = 32, 0.37 otherwise), and one key whose scores carry +60 (probability 1 to fp32).  Finite, and within 4 x the error
    of torch's fp32 evaluation of the same formulas on the CPU (floored at 2^-24 max|ref|), per output.

    Measured (max abs error against float64; yardstick = torch fp32 on the CPU, the bar is 4 x yardstick):
      yardstick, worst case of each kind over d and plain / split (out, dq, dk, dv, lse):
        big     3.1e-5, 1.8e-4, 1.2e-4, 2.6e-5, 3.9e-5   (d = 128; 1.8e-5 .. 4.5e-5 at d = 32)
        scale   5.9e-6, 2.1e-5, 2.0e-5, 5.8e-6, 8.2e-6
        offset  0 (floor 1.3e-7 .. 1.9e-7), 8.6e-5, 2.6e-5, 1.0e-5, 6.6e-5   (the true dq / dk are ~1e-14 there: what is
                measured is the cancellation residue of dP - Delta, which every fp32 evaluation of the formula has)
      kernel: printed by the test next to the yardstick (no GPU figures recorded yet)
    """
    name, b, h, sq, sk, d, kind, scale, spec = case
    q, k, v, dout, mask = _case(name, b, h, sq, sk, d, kind, scale, spec)
    ref = ar.attention_ref(q, k, v, mask, scale, dout)
    y32 = ar.attention_ref(q, k, v, mask, scale, dout, dtype=torch.float32)
    got = run_kernels(q, k, v, dout, mask, scale)
    assert_finite(got)
    assert_contract_on_dead_rows(got, mask)
    e, ey = errors(got, ref), errors(y32, ref)
    worst = []
    for n in OUTPUTS + ("lse",):
        floor = 2.0 ** -24 * ref[n][torch.isfinite(ref[n])].abs().max().item()
        yard = max(ey[n], floor)
        print(f"\n[attention extreme {name}] {n}: kernel {e[n]:.2e}, fp32 yardstick {ey[n]:.2e} (floor {floor:.1e}), "
              f"bar {YARD_FACTOR * yard:.2e}", end="")
        if not e[n] <= YARD_FACTOR * yard:
            worst.append((n, e[n], yard))
    print()
    assert not worst, (name, worst)


# ---------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("d", ar.DS)
def test_split_variants_are_bit_identical_run_to_run(d):
    """The split kernels merge their four partials in the fixed order wave 0..3 (no atomics): the same call twice gives
    the same bits."""
    b, h, sq, sk = ar.GEO["split"]
    assert ar.variants(b, h, sq, sk, d) == {(p, "split", d) for p in ("fwd", "dq", "dkv")}
    q, k, v, dout, mask = _case(f"determinism-d{d}", b, h, sq, sk, d, "randn", None, ("random",))
    first = run_kernels(q, k, v, dout, mask, None)
    second = run_kernels(q, k, v, dout, mask, None)
    for n in OUTPUTS + ("lse",):
        assert torch.equal(first[n], second[n]), n


# ---------------------------------------------------------------------------------------------- BERT at real lengths
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("s", [64, 128])
def test_bert_two_layers_with_whole_key_tiles_of_padding(s, precision):
    """Sentences of 5, 33 and S tokens in S = 64 / 128 slots: whole 32-key tiles are padding, as they are in use (S = 128
    runs the split kernels).  Two layers against the oracle, the encoder's 5e-4 bar on the valid tokens."""
    import oracle
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.text_encoder import BertEncoderHIP
    bsd = synth.make_state_dict(synth.bert_spec("", layers=2), seed=52)
    enc = BertEncoderHIP(num_hidden_layers=2)
    assert set(enc.state_dict()) == set(bsd)
    enc.load_state_dict(bsd, strict=True)
    enc.precision = precision
    enc = enc.cuda().eval()
    ids, mask = synth.make_token_ids(3, s, seed=90 + s, pad_from=[5, 33, s])
    tok = enc(ids, mask).cpu()
    assert bool(torch.isfinite(tok).all())
    with torch.no_grad():
        ref = oracle.bert_token_features(ids, mask, bsd, num_layers=2)
    valid = mask.bool()
    err = (tok - ref)[valid].abs().max().item()
    print(f"\n[bert 2 layers S={s} {precision}] max err on valid tokens {err:.2e}")
    assert err < 5e-4
