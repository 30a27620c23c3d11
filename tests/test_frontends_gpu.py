"""The encoder front ends of csrc/encoders.hip called directly: ops.logmel, ops.frame_examples, ops.bert_embed_ln and
ops.add_inplace at the inputs the encoders never feed them -- silence, full-scale PCM, one frame, no padding, windows at the
last frame, widths that are not a multiple of 64, constant rows, ids outside the table -- and the host-side refusals.

Bars.  log-mel keeps the front end's 2e-5 on the log values, against the oracle's float64 numpy.  Framing and the in-place
add are bit-exact against torch.  The embedding LayerNorm has no fixed bar: the yardstick is torch's fp32 F.layer_norm on
the CPU on the same fp32 sums word + pos + type, its max abs error against float64 floored at 2^-24 max|ref|, and the kernel
is allowed 4 x that (two fp32 LayerNorms that sum a row in different orders).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LOGMEL_BAR = 2e-5


# ---------------------------------------------------------------------------------------------- log-mel
def _mel():
    from feature_vs_text_compound_emotion_amd.audio_backbone import mel_matrix
    return torch.from_numpy(mel_matrix()).cuda().contiguous()


def _logmel_ref(pcm_row, pad):
    """The reference's front end in float64 numpy with ``pad`` edge samples (the oracle pads a fixed second)."""
    import oracle.vggish as ov
    x = np.asarray(pcm_row).astype(np.float64) / 32768.0
    return ov.log_mel_spectrogram(np.pad(x, (0, pad), "edge"))


def _tone(n, hz, amp=20000.0):
    t = np.arange(n) / 16000.0
    return torch.from_numpy(np.round(amp * np.sin(2 * np.pi * hz * t)).astype(np.int16))


def _noise(n, seed, amp=3000.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.clamp(torch.round(torch.randn(n, generator=g) * amp), -32768, 32767).to(torch.int16)
    x[-1] = 12345          # the sample the edge padding repeats
    return x


def _check_logmel(pcm, pad, what):
    from feature_vs_text_compound_emotion_amd import ops
    pcm = pcm if pcm.dim() == 2 else pcm[None]
    got = ops.logmel(pcm.cuda().contiguous(), pad, _mel(), 0.01).cpu().numpy()
    for i in range(pcm.shape[0]):
        ref = _logmel_ref(pcm[i].numpy(), pad)
        assert got[i].shape == ref.shape, (what, got[i].shape, ref.shape)
        err = np.abs(got[i] - ref).max()
        print(f"\n[logmel {what} clip {i}] frames {ref.shape[0]} max err {err:.2e}", end="")
        assert np.isfinite(got[i]).all() and err < LOGMEL_BAR, (what, i, err)
    return got


def test_logmel_of_silence_is_log_of_the_offset_exactly():
    got = _check_logmel(torch.zeros(2, 1600, dtype=torch.int16), 160, "silence")
    assert got.shape == (2, 9, 64)
    assert (got == np.float32(np.log(0.01))).all()


def test_logmel_full_scale_square_wave():
    x = torch.full((4000,), 32767, dtype=torch.int16)
    x[(torch.arange(4000) // 25) % 2 == 1] = -32768
    assert int(x.min()) == -32768 and int(x.max()) == 32767
    _check_logmel(x, 160, "square")


def test_logmel_single_impulse():
    x = torch.zeros(2400, dtype=torch.int16)
    x[1000] = 20000
    _check_logmel(x, 0, "impulse")


@pytest.mark.parametrize("hz", [1000.0, 1015.625])      # bin 32 of the 512-point DFT (31.25 Hz apart), and bin 32.5
def test_logmel_tone_on_and_between_bin_centres(hz):
    _check_logmel(_tone(3200, hz), 160, f"tone {hz}")


def test_logmel_exactly_one_frame_and_too_short_inputs():
    from feature_vs_text_compound_emotion_amd import ops
    got = _check_logmel(_noise(400, 3), 0, "one frame")
    assert got.shape == (1, 1, 64)
    got = _check_logmel(_noise(240, 4), 160, "one frame, 160 of it padding")
    assert got.shape == (1, 1, 64)
    for n, pad in ((399, 0), (300, 99), (1, 398)):
        with pytest.raises(ValueError):
            ops.logmel(_noise(n, 5)[None].cuda(), pad, _mel(), 0.01)


@pytest.mark.parametrize("pad", [0, 160, 16000])
def test_logmel_edge_padding_over_zero_one_and_many_frames(pad):
    got = _check_logmel(_noise(1680, 6), pad, f"pad {pad}")
    assert got.shape[1] == 1 + (1680 + pad - 400) // 160


def test_logmel_three_clips_of_different_content_in_one_call():
    from feature_vs_text_compound_emotion_amd import ops
    n = 2000
    sq = torch.full((n,), 32767, dtype=torch.int16)
    sq[(torch.arange(n) // 40) % 2 == 1] = -32768
    pcm = torch.stack([_noise(n, 7), _tone(n, 440.0), sq])
    got = _check_logmel(pcm, 160, "three clips")
    for i in range(3):      # each clip alone gives the same bits: no clip reads its neighbour
        alone = ops.logmel(pcm[i:i + 1].cuda().contiguous(), 160, _mel(), 0.01).cpu().numpy()
        assert np.array_equal(alone[0], got[i])


# ---------------------------------------------------------------------------------------------- example framing
@pytest.mark.parametrize("win", [1, 50, 96])
def test_frame_examples_is_bit_exact_against_torch_indexing(win):
    from feature_vs_text_compound_emotion_amd import ops
    clips, frames = 3, 150
    lm = torch.randn(clips, frames, 64, generator=torch.Generator().manual_seed(win)).cuda()
    last = frames - win
    for starts in ([0], [last], [0, last], [0, 1, 2, 5, 5, last - 1, last, 3], list(range(0, last + 1))):
        want = torch.stack([lm[:, s:s + win] for s in starts], 1)
        for given in (starts, torch.tensor(starts), torch.tensor(starts, dtype=torch.int32)):
            got = ops.frame_examples(lm, given, win)
            assert tuple(got.shape) == (clips, len(starts), win, 64) and torch.equal(got, want), (win, starts[:4])


def test_frame_examples_refuses_starts_outside_the_logmel_before_any_launch():
    from feature_vs_text_compound_emotion_amd import ops
    frames, win = 150, 96
    lm = torch.randn(2, frames, 64, generator=torch.Generator().manual_seed(1)).cuda()
    for bad in ([-1], [0, frames - win + 1], [frames], [0, 10, 2 ** 31 - 1], []):
        with pytest.raises(ValueError):
            ops.frame_examples(lm, bad, win)
    with pytest.raises(ValueError):
        ops.frame_examples(lm, [0], frames + 1)
    with pytest.raises(ValueError):       # device starts cannot be checked without a synchronisation
        ops.frame_examples(lm, torch.tensor([0], dtype=torch.int32).cuda(), win)


def test_wav_to_examples_is_the_checked_gather_of_the_logmel():
    """VGGish.wav_int16_to_examples hands example_starts' host list to the checked wrapper: same bits as indexing."""
    from feature_vs_text_compound_emotion_amd import ops, synth
    from feature_vs_text_compound_emotion_amd.audio_backbone import VGGish, example_starts
    net = VGGish().cuda()
    pcm = torch.stack([synth.make_audio_int16(0.73, 16000, seed=s) for s in (1, 2)])
    ex = net.wav_int16_to_examples(pcm, 16000, 0.96, 0.05)
    lm = ops.logmel(pcm.cuda().contiguous(), 16000, _mel(), 0.01)
    starts = example_starts(lm.shape[1], 96, 5.0)
    assert len(starts) > 1 and starts[-1] + 96 <= lm.shape[1]
    assert torch.equal(ex, torch.stack([lm[:, s:s + 96] for s in starts], 1))


# ---------------------------------------------------------------------------------------------- BERT embeddings + LayerNorm
def _embed_tables(vocab, max_pos, hd, seed, mean=0.0, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    word = mean + spread * torch.randn(vocab, hd, generator=g)
    pos = spread * torch.randn(max_pos, hd, generator=g)
    typ = spread * torch.randn(2, hd, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(hd, generator=g)
    beta = 0.1 * torch.randn(hd, generator=g)
    return word, pos, typ, gamma, beta


def _embed_check(ids, tables, eps, what):
    """Kernel vs float64 LayerNorm of the fp32 sums (word + pos) + type, under 4 x torch's fp32 F.layer_norm's own error."""
    from feature_vs_text_compound_emotion_amd import ops
    word, pos, typ, gamma, beta = tables
    b, s = ids.shape
    hd = word.shape[1]
    x = (word[ids] + pos[:s][None]) + typ[0][None, None]          # fp32, the kernel's order of the two additions
    ref = F.layer_norm(x.double(), (hd,), gamma.double(), beta.double(), eps)
    yard = (F.layer_norm(x, (hd,), gamma, beta, eps).double() - ref).abs().max().item()
    floor = 2.0 ** -24 * ref.abs().max().item()
    got = ops.bert_embed_ln(ids.cuda(), *(t.cuda().contiguous() for t in tables), eps).cpu()
    assert tuple(got.shape) == (b, s, hd) and bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs().max().item()
    bar = 4.0 * max(yard, floor)
    print(f"\n[bert_embed_ln {what}] kernel {err:.2e}, torch fp32 layer_norm {yard:.2e} (floor {floor:.1e}), bar {bar:.2e}")
    assert err <= bar, (what, err, yard, floor)
    return got


@pytest.mark.parametrize("hd", [768, 128, 100, 32])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
def test_bert_embed_ln_widths_and_eps(hd, eps):
    """hidden 100 and 32 leave lanes without a column (lane >= Hd) and are not multiples of 64; 3 x 7 = 21 tokens are not a
    multiple of the four tokens per block.

    Measured (max abs error against float64; the bar is 4 x the yardstick):
      yardstick (torch fp32 F.layer_norm): 2.6e-7 .. 5.9e-7 over the widths and eps here; 6.0e-3 on the rows of mean 1e3 and
      spread 1e-2 (the fp32 mean is good to 6e-5, the spread is 1e-2)
      kernel: printed by the test next to the yardstick (no GPU figures recorded yet)
    """
    vocab, max_pos = 97, 16
    tables = _embed_tables(vocab, max_pos, hd, seed=hd)
    ids = torch.randint(0, vocab, (3, 7), generator=torch.Generator().manual_seed(hd + 1))
    ids[0, 0], ids[2, 6] = 0, vocab - 1
    _embed_check(ids, tables, eps, f"hidden {hd} eps {eps:g}")


def test_bert_embed_ln_sequence_as_long_as_the_position_table_and_longer():
    from feature_vs_text_compound_emotion_amd import ops
    vocab, max_pos, hd = 50, 12, 128
    tables = _embed_tables(vocab, max_pos, hd, seed=9)
    ids = torch.randint(0, vocab, (2, max_pos), generator=torch.Generator().manual_seed(2))
    _embed_check(ids, tables, 1e-12, "S == max_pos")
    long_ids = torch.randint(0, vocab, (2, max_pos + 1), generator=torch.Generator().manual_seed(3))
    with pytest.raises(RuntimeError, match="position table"):
        ops.bert_embed_ln(long_ids.cuda(), *(t.cuda().contiguous() for t in tables), 1e-12)


@pytest.mark.parametrize("hd", [768, 100])
def test_bert_embed_ln_constant_row_returns_beta_exactly(hd):
    """word + pos + type constant over the row: variance 0 under eps 1e-12.  The constants are dyadic (0.5 + 0.25 + 0.125),
    so every partial sum and the mean are exact in fp32 in any order; x - mean is then exactly 0 and y must be beta, not
    0 * rsqrt(1e-12) noise."""
    from feature_vs_text_compound_emotion_amd import ops
    g = torch.Generator().manual_seed(4)
    word = torch.randn(5, hd, generator=g)
    word[3] = 0.5
    pos = torch.full((4, hd), 0.25)
    typ = torch.full((2, hd), 0.125)
    gamma, beta = 1.0 + torch.randn(hd, generator=g), torch.randn(hd, generator=g)
    ids = torch.tensor([[3, 1, 3, 3]])
    got = ops.bert_embed_ln(ids.cuda(), word.cuda(), pos.cuda(), typ.cuda(), gamma.cuda(), beta.cuda(), 1e-12).cpu()
    assert bool(torch.isfinite(got).all())
    for tok in (0, 2, 3):
        assert torch.equal(got[0, tok], beta), tok
    assert not torch.equal(got[0, 1], beta)


def test_bert_embed_ln_rows_with_a_large_mean_and_a_small_spread():
    """Rows of mean 1e3 and spread 1e-2: the mean has to be subtracted before the squares are summed."""
    vocab, max_pos, hd = 40, 8, 768
    tables = _embed_tables(vocab, max_pos, hd, seed=11, mean=1e3, spread=1e-2)
    ids = torch.randint(0, vocab, (2, 8), generator=torch.Generator().manual_seed(12))
    _embed_check(ids, tables, 1e-12, "mean 1e3 spread 1e-2")


def test_bert_embed_ln_clamps_ids_outside_the_table():
    """include/cer_hip.h documents the clamp: id < 0 reads row 0, id >= vocab reads row vocab - 1."""
    from feature_vs_text_compound_emotion_amd import ops
    vocab, hd = 30, 128
    tables = [t.cuda().contiguous() for t in _embed_tables(vocab, 8, hd, seed=13)]
    bad = torch.tensor([[-1, vocab, 5, -(2 ** 40), 2 ** 40, vocab - 1, 0]])
    good = torch.tensor([[0, vocab - 1, 5, 0, vocab - 1, vocab - 1, 0]])
    assert torch.equal(ops.bert_embed_ln(bad.cuda(), *tables, 1e-12), ops.bert_embed_ln(good.cuda(), *tables, 1e-12))


def test_bert_encoder_raises_on_host_ids_outside_the_vocabulary():
    """nn.Embedding raises on such ids; BertEncoderHIP restates that for ids that arrive on the host (no synchronisation)."""
    from feature_vs_text_compound_emotion_amd.text_encoder import BertEncoderHIP
    enc = BertEncoderHIP(vocab_size=50, hidden_size=128, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256,
                         max_position_embeddings=16).cuda().eval()
    ok = torch.tensor([[1, 49, 0, 7]])
    assert tuple(enc(ok, torch.ones_like(ok), last_n_sum=1).shape) == (1, 4, 128)
    for bad in (torch.tensor([[1, 50, 0, 7]]), torch.tensor([[1, -1, 0, 7]])):
        with pytest.raises(ValueError):
            enc(bad, torch.ones_like(bad), last_n_sum=1)


# ---------------------------------------------------------------------------------------------- y += x
@pytest.mark.parametrize("n", [4, 1028, 3 * 7 * 768, 256 * 1024 + 4])
def test_add_inplace_is_exact(n):
    from feature_vs_text_compound_emotion_amd import ops
    g = torch.Generator().manual_seed(n)
    y, x = torch.randn(n, generator=g) * 100.0, torch.randn(n, generator=g)
    yd, xd = y.cuda(), x.cuda()
    got = ops.add_inplace(yd, xd)
    assert got.data_ptr() == yd.data_ptr() and torch.equal(yd.cpu(), y + x) and torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("n", [1, 6, 1023])
def test_add_inplace_rejects_sizes_that_are_not_a_multiple_of_four(n):
    from feature_vs_text_compound_emotion_amd import ops
    y, x = torch.zeros(n).cuda(), torch.ones(n).cuda()
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.add_inplace(y, x)
    assert bool((y == 0).all())
