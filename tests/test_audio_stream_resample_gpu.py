"""The streaming resampler on the GPU: PCM at any rate and channel count pushed in chunks through ``LogMelStream(resample=...)``
gives, bit for bit, the examples ``VGGish.wav_int16_to_examples(..., resample=...)`` gives the whole signal.  The offline kernel
and the stream run one device function per output (csrc/resample_row.h) and one per row (csrc/logmel_row.h), so every
comparison with the offline path is for equality; the bar against the independent float64 reference is the offline path's own
in tests/test_resample_gpu.py."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN, HOP = 96, 0.025
# rate, filter, channels, seconds: downsampling by 3 and by 441 / 160, upsampling, the identity table, and 192 kHz, where the
# 256 outputs of a block read 3072 + T inputs, more than one 2048-sample LDS window
CONFIGS = {"48k-fast-mono": (48000, "kaiser_fast", 1, 1.05), "48k-best-stereo": (48000, "kaiser_best", 2, 0.5),
           "44k1-fast-3ch": (44100, "kaiser_fast", 3, 0.5), "8k-fast-mono": (8000, "kaiser_fast", 1, 1.3),
           "16k-stereo": (16000, "kaiser_best", 2, 1.1), "192k-fast-mono": (192000, "kaiser_fast", 1, 0.3)}


def _pkg():
    from feature_vs_text_compound_emotion_amd import audio_stream, ops, synth
    return audio_stream, ops, synth


@functools.lru_cache(maxsize=None)
def _vggish():
    from feature_vs_text_compound_emotion_amd.audio_backbone import VGGish
    return VGGish().cuda()


@functools.lru_cache(maxsize=None)
def _signal(seconds, rate, channels, seed):
    """int16 [n] for one channel, interleaved [n, C] for more."""
    synth = _pkg()[2]
    chans = [synth.make_audio_int16(seconds, rate, seed=seed + 100 * ch) for ch in range(channels)]
    return chans[0] if channels == 1 else torch.stack(chans, dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def _offline(seconds, rate, channels, seed, filter, hop_sec):
    """Offline examples [n, 96, 64] of one signal, computed once and shared."""
    pcm = _signal(seconds, rate, channels, seed)
    return _vggish().wav_int16_to_examples(pcm[None], rate, 0.96, hop_sec, resample=filter)[0]


def _chunks(n, max_chunk, seed):
    rng, out = random.Random(seed), []
    while n:
        out.append(min(n, rng.randint(1, max_chunk)))
        n -= out[-1]
    return out


def _push_alone(stream, pcm, chunks, s=0):
    """One signal through stream ``s`` while the other streams rest: (examples before finish, all examples)."""
    parts, at = [], 0
    for c in chunks:
        counts = [0] * stream.streams
        counts[s] = c
        ex, emitted = stream.push(pcm[at:at + c], counts)
        assert sum(emitted) == emitted[s] == ex.shape[0] and tuple(ex.shape[1:]) == (WIN, 64)
        parts.append(ex)
        at += c
    assert at == pcm.shape[0]
    before = torch.cat(parts)
    ex, emitted = stream.finish([s])
    assert sum(emitted) == emitted[s] == ex.shape[0]
    return before, torch.cat([before, ex])


# ---------------------------------------------------------------------------------------------- one stream, any chunking
CHUNKINGS = {"one-chunk": lambda n: ([n], n), "37s": lambda n: ([37] * (n // 37) + ([n % 37] if n % 37 else []), 4096),
             "random": lambda n: (_chunks(n, 4096, 5), 4096), "max-100": lambda n: (_chunks(n, 100, 6), 100)}


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_one_stream_equals_offline_under_any_chunking(config, chunking):
    audio_stream = _pkg()[0]
    rate, filter, channels, seconds = CONFIGS[config]
    pcm = _signal(seconds, rate, channels, 7)
    ref = _offline(seconds, rate, channels, 7, filter, HOP)
    chunks, max_samples = CHUNKINGS[chunking](pcm.shape[0])
    stream = audio_stream.LogMelStream(1, HOP, max_samples=max_samples, sample_rate=rate, channels=channels, resample=filter)
    before, full = _push_alone(stream, pcm, chunks)
    assert stream.samples_seen == [0] and stream.resampled == [0] and stream.examples_emitted == [0]     # finish resets
    if chunking == "max-100":       # both rings wrapped many times
        assert pcm.shape[0] > 4 * stream.ring_inputs and (pcm.shape[0] + rate) * 16000 // rate > 4 * stream.ring_samples
    # what is out before finish is a prefix of the offline examples: those whose rows the complete outputs hold
    done = audio_stream.outputs_complete(pcm.shape[0], stream.L, stream.M, stream.T)
    n_before = len([e for e in range(ref.shape[0]) if round(HOP * 100 * e) + WIN <= audio_stream.num_rows(done)])
    assert before.shape[0] == n_before and torch.equal(before, ref[:n_before])
    assert n_before > 0 or seconds < 1.0
    assert full.shape == ref.shape and ref.shape[0] > 10 and torch.equal(full, ref)


# ---------------------------------------------------------------------------------------------- ragged streams
RAGGED = dict(rate=44100, filter="kaiser_fast", channels=2, seconds=0.4, seeds=(31, 32, 33, 34, 35), max_samples=700, hop=1 / 30)


def _ragged_ticks(total, streams, max_samples, seed, late=(3, 6), lonely_every=7):
    """Per-stream counts in 0 .. max_samples per tick until every stream has had ``total`` frames; stream ``late[0]`` joins
    after ``late[1]`` ticks; every ``lonely_every``-th tick brings one frame to one stream."""
    rng, fed, ticks = random.Random(seed), [0] * streams, []
    while min(fed) < total:
        tick = len(ticks)
        open_ = [s for s in range(streams) if fed[s] < total and not (s == late[0] and tick < late[1])]
        counts = [0] * streams
        if tick % lonely_every == lonely_every - 1:
            if open_:
                counts[rng.choice(open_)] = 1
        else:
            for s in open_:
                counts[s] = min(rng.randint(0, max_samples), total - fed[s])
        fed = [f + c for f, c in zip(fed, counts)]
        ticks.append(counts)
    return ticks


def _drive(stream, pcm, ticks, total):
    """pcm [S][total(, C)] through ``stream`` tick by tick; a stream is finished at the tick its last frame arrives."""
    streams = len(pcm)
    fed, outs, done = [0] * streams, [[] for _ in range(streams)], {}

    def unpack(ex, counts):
        at = 0
        for s, c in enumerate(counts):
            outs[s].append(ex[at:at + c])
            at += c
        assert at == ex.shape[0]

    for tick, counts in enumerate(ticks):
        unpack(*stream.push(torch.cat([pcm[s][fed[s]:fed[s] + c] for s, c in enumerate(counts)]), counts))
        fed = [f + c for f, c in zip(fed, counts)]
        ending = [s for s in range(streams) if fed[s] == total and s not in done]
        if ending:
            unpack(*stream.finish(ending))
            done.update({s: tick for s in ending})
    return [torch.cat(o) for o in outs], done


def test_ragged_streams_equal_offline_and_each_stream_alone():
    audio_stream = _pkg()[0]
    r = RAGGED
    pcm = [_signal(r["seconds"], r["rate"], r["channels"], s) for s in r["seeds"]]
    total = pcm[0].shape[0]
    kw = dict(max_samples=r["max_samples"], sample_rate=r["rate"], channels=r["channels"], resample=r["filter"])
    ticks = _ragged_ticks(total, len(pcm), r["max_samples"], seed=77)
    stream = audio_stream.LogMelStream(len(pcm), r["hop"], **kw)
    outs, done = _drive(stream, pcm, ticks, total)
    assert len(set(done.values())) > 1                                  # streams end at different ticks
    assert any(sum(c) == 1 for c in ticks) and all(c[3] == 0 for c in ticks[:6])
    for s, seed in enumerate(r["seeds"]):
        ref = _offline(r["seconds"], r["rate"], r["channels"], seed, r["filter"], r["hop"])
        assert outs[s].shape == ref.shape and ref.shape[0] > 10 and torch.equal(outs[s], ref), s
        alone = audio_stream.LogMelStream(1, r["hop"], **kw)
        _, full = _push_alone(alone, pcm[s], [c[s] for c in ticks if c[s]])
        assert torch.equal(full, outs[s]), s


# ---------------------------------------------------------------------------------------------- reset and re-use
def test_reset_and_reuse_equal_a_fresh_stream():
    audio_stream = _pkg()[0]
    rate, filter, channels, seconds, max_samples = 48000, "kaiser_fast", 2, 0.4, 700
    a, b, c = (_signal(seconds, rate, channels, s) for s in (51, 52, 53))
    ref = [_offline(seconds, rate, channels, s, filter, HOP) for s in (51, 52, 53)]
    n, half = a.shape[0], 9000
    stream = audio_stream.LogMelStream(2, HOP, max_samples=max_samples, sample_rate=rate, channels=channels, resample=filter)
    at = 0
    for k in _chunks(half, max_samples, 1):          # both streams half way through a and b ...
        stream.push(torch.cat([a[at:at + k], b[at:at + k]]), [k, k])
        at += k
    stream.reset([0])                                # ... stream 0 drops a and starts c, stream 1 goes on with b
    assert stream.samples_seen == [0, half] and stream.resampled[0] == 0 and stream.resampled[1] > 0
    outs, fed = [[], []], [0, half]
    for k in _chunks(n - half, max_samples, 2):
        ex, counts = stream.push(torch.cat([c[fed[0]:fed[0] + k], b[fed[1]:fed[1] + k]]), [k, k])
        outs[0].append(ex[:counts[0]])
        outs[1].append(ex[counts[0]:])
        fed = [f + k for f in fed]
    ex, counts = stream.finish([1])                  # b is complete
    outs[1].append(ex)
    assert counts[0] == 0 and torch.equal(torch.cat(outs[1]), ref[1])
    for k in _chunks(half, max_samples, 3):
        ex, counts = stream.push(c[fed[0]:fed[0] + k], [k, 0])
        outs[0].append(ex)
        fed[0] += k
    outs[0].append(stream.finish([0])[0])
    assert torch.equal(torch.cat(outs[0]), ref[2])
    _, again = _push_alone(stream, a, _chunks(n, max_samples, 4), s=1)      # stream 1 re-used after finish
    assert torch.equal(again, ref[0])


# ---------------------------------------------------------------------------------------------- the resampler alone
@pytest.mark.parametrize("rate,filter,channels", [(44100, "kaiser_fast", 2), (48000, "kaiser_best", 1)])
def test_ring_holds_the_offline_samples_across_the_2_30_wrap(rate, filter, channels):
    """The mix-append and resample kernels alone, driven by the pure schedule with the host ints of a stream that has already
    had M (2^30 - d) frames: a whole number of periods of the phase, so output L (2^30 - d) + i sits where output i of a fresh
    signal sits, and the input and the output positions both pass a multiple of 2^30 within the signal.  The ring's slots
    behind the first frame are zero, as the inputs before a signal are."""
    audio_stream, ops, _ = _pkg()
    from feature_vs_text_compound_emotion_amd.audio_backbone import resample_taps, resampled_length
    pcm = _signal(0.3, rate, channels, 61).cuda()
    taps_h, L, M = resample_taps(rate, filter)
    taps, T = torch.from_numpy(taps_h).cuda().contiguous(), taps_h.shape[1]
    n_in, d, max_samples = pcm.shape[0], 100, 1500
    f0, n_base = M * ((1 << 30) - d), L * ((1 << 30) - d)
    n_out = resampled_length(n_in + rate, rate)
    assert f0 % (1 << 30) + n_in + rate > (1 << 30) and n_base % (1 << 30) + n_out > (1 << 30)
    rin, rs = audio_stream.resample_ring_sizes(WIN, max_samples, L, M, T)[0], 32768
    assert n_out + T < rs and n_in + rate > 4 * rin
    in_ring = torch.zeros((1, rin), device="cuda", dtype=torch.float64)
    out_ring = torch.zeros((1, rs), device="cuda", dtype=torch.float64)
    done = audio_stream.outputs_complete(f0, L, M, T)
    state = (f0, done, audio_stream.num_rows(done), 1)      # rows and examples are not run here: one example, a hop without end
    steps, at = [], 0
    for c in _chunks(n_in, max_samples, 9):
        steps.append((c, at))
        at += c
    steps += [(c, None) for c in audio_stream.pad_chunks(max_samples, rate)] + [(0, None)]
    for count, offset in steps:
        final = n_base + n_out if count == 0 else None
        state, mix, out, _, _ = audio_stream.resampled_step(state, count, offset, L, M, T, WIN, 1e15, None, final)
        mix_t, out_t, _, _ = ops.resample_stream_tables([(0,) + mix] if mix else [], [(0,) + out] if out else [], [], [], "cuda")
        if mix_t is not None:
            ops.resample_stream_append(pcm, mix_t, count, T - 1, in_ring)
        if out_t is not None:
            ops.resample_stream_outputs(in_ring, out_t, out[1], taps, L, M, out_ring)
    assert state[:2] == (f0 + n_in + rate, n_base + n_out)
    got = out_ring[0, (n_base + torch.arange(n_out, device="cuda")) % rs]
    want = ops.resample_pcm(pcm[None].contiguous(), channels > 1, rate, taps, L, M, n_out)[0]
    assert torch.equal(got, want) and float(want.abs().max()) > 0.01


# ---------------------------------------------------------------------------------------------- an independent reference
def test_streamed_examples_match_the_independent_float64_reference():
    """Bar 2e-5: the offline path's own against this reference (tests/test_resample_gpu.py).  Measured: 2.5e-07."""
    import resample_ref as R
    audio_stream = _pkg()[0]
    rate, channels, filter, hop = 44100, 2, "kaiser_best", 0.05
    pcm = _signal(0.4, rate, channels, 91)
    ref = R.wav_to_examples_ref(pcm.numpy(), rate, channels, filter, 0.96, hop)
    stream = audio_stream.LogMelStream(1, hop, max_samples=1000, sample_rate=rate, channels=channels, resample=filter)
    _, full = _push_alone(stream, pcm, _chunks(pcm.shape[0], 1000, 3))
    err = np.abs(full.cpu().numpy() - ref).max() if tuple(full.shape) == ref.shape else float("nan")
    print(f"streamed 44.1 kHz stereo vs the float64 reference: max abs {err:.3e}")
    assert tuple(full.shape) == ref.shape and err < 2e-5


# ---------------------------------------------------------------------------------------------- end to end
def test_48_khz_stereo_pcm_to_logits_equals_the_offline_forward():
    from feature_vs_text_compound_emotion_amd import synth
    from feature_vs_text_compound_emotion_amd.streaming import LFANStream, stream_forward
    from test_tail_gpu import _build_lfan
    audio_stream = _pkg()[0]
    mods, seconds, hop, seeds, ncls, rate, filter = ["logmel"], 0.3, 0.1, (81, 82), 7, 48000, "kaiser_fast"
    spec, alias = synth.lfan_spec(mods, n_cls=ncls)
    model = _build_lfan(mods, synth.make_state_dict(spec, alias, seed=5), 4, n_cls=ncls).eval()
    pcm = torch.stack([_signal(seconds, rate, 2, s) for s in seeds])
    offline = model.spatial["audio"].backbone.wav_int16_to_examples(pcm, rate, 0.96, hop, resample=filter)
    assert tuple(offline.shape) == (2, 4, 96, 64)
    with torch.no_grad():
        ref = stream_forward(model, {"logmel": offline.permute(0, 3, 1, 2).contiguous()})
    total = pcm.shape[1]
    for seed, together in ((1, True), (2, False)):
        audio = audio_stream.LogMelStream(2, hop, max_samples=3000, sample_rate=rate, channels=2, resample=filter)
        lfan = LFANStream(model, 2)
        logits = [[], []]

        def feed(examples, counts):
            if sum(counts):
                out, at = lfan.push_ragged({"logmel": examples.transpose(1, 2)}, counts), 0
                for s, c in enumerate(counts):
                    logits[s].append(out[at:at + c])
                    at += c

        fed, rng = [0, 0], random.Random(seed)
        while min(fed) < total:
            counts = [min(rng.randint(0, 3000), total - f) for f in fed]
            feed(*audio.push(torch.cat([pcm[s, fed[s]:fed[s] + c] for s, c in enumerate(counts)]), counts))
            fed = [f + c for f, c in zip(fed, counts)]
        for group in ([None] if together else [[1], [0]]):
            feed(*audio.finish(group))
        got = torch.stack([torch.cat(rows) for rows in logits])
        assert got.shape == ref.shape and torch.equal(got, ref), seed


# ---------------------------------------------------------------------------------------------- tables are clamped
def test_wrong_tables_stay_inside_the_rings_and_the_packed_input():
    """Rings and packed input sit in the middle of larger allocations, between guard slabs of one whole stream's ring (one
    ``max_count`` of input frames) filled with a sentinel.  Every wrong stream index and every wrong offset is within one slab
    of the valid range, so even a kernel without that clamp would land in a guard; positions, counts and tap rows are wrong by
    any amount, which the masks, the cut to ``max_count`` and the reduction modulo L (read in the kernels, and emulated in
    tests/test_audio_stream_resample_cpu.py) keep inside."""
    _, ops, _ = _pkg()
    from feature_vs_text_compound_emotion_amd.audio_backbone import resample_taps
    S, rin, rs, C, max_count, m = 2, 1024, 512, 2, 256, 300
    taps_h, L, M = resample_taps(44100, "kaiser_fast")
    T = taps_h.shape[1]
    sent16, sentd = 23130, 12345.0
    big_in = torch.full(((S + 2) * rin,), sentd, device="cuda", dtype=torch.float64)
    big_out = torch.full(((S + 2) * rs,), sentd, device="cuda", dtype=torch.float64)
    big_pcm = torch.full(((m + 2 * max_count) * C,), sent16, device="cuda", dtype=torch.int16)
    big_taps = torch.full(((L + 2 * 8) * T,), sentd, device="cuda", dtype=torch.float64)
    in_ring = big_in[rin:(S + 1) * rin].view(S, rin)
    out_ring = big_out[rs:(S + 1) * rs].view(S, rs)
    packed = big_pcm[max_count * C:(max_count + m) * C].view(m, C)
    taps = big_taps[8 * T:(8 + L) * T].view(L, T)
    in_ring.zero_()
    out_ring.zero_()
    packed.copy_(_signal(0.1, 44100, C, 73)[:m])
    taps.copy_(torch.from_numpy(taps_h))
    mixed = (packed.double() / 32768.0).sum(1) / C        # two channels: one rounding-free sum, then an exact halving
    big = 1 << 30
    # stream indices -1 and S, offsets past the packed input by less than one max_count, a count above max_count, a repeat
    mix_t = torch.tensor([[-1, S, 0, 1], [100, big - 24, 500, 0], [200, 200, 200, 1000], [0, m + 10, m - 50, -1]],
                         dtype=torch.int32, device="cuda")
    ops.resample_stream_append(packed, mix_t, max_count, T - 1, in_ring)
    torch.cuda.synchronize()
    assert torch.equal(in_ring[0, 100:300], mixed[:200])                                  # -1 is stream 0
    assert bool((in_ring[S - 1, rin - 24:] == 0).all()) and bool((in_ring[S - 1, :176] == 0).all())   # S is S - 1; reads past the input are 0
    assert torch.equal(in_ring[0, 500:550], mixed[m - 50:]) and bool((in_ring[0, 550:700] == 0).all())
    before = in_ring.clone()
    # outputs: stream -1 and S, positions anywhere, a count above max_count, tap rows >= L and < 0, ranges anywhere
    out_t = torch.tensor([[-1, S, 1, 0], [5, big - 7, -big, 2 * big - 1], [max_count, 10 * max_count, 2 * big - 1, 3],
                          [L + 3, 7 * L, -5, 2 * big - 1], [100, big - 1, -big, 2 * big - 1],
                          [-40, -2 * big, 2 * big - 1, -2 * big], [200, 2 * big - 1, -2 * big, 2 * big - 1]],
                         dtype=torch.int32, device="cuda")
    ops.resample_stream_outputs(in_ring, out_t, max_count, taps, L, M, out_ring)
    torch.cuda.synchronize()
    for bigt, lo, hi, sent in ((big_in, rin, (S + 1) * rin, sentd), (big_out, rs, (S + 1) * rs, sentd),
                               (big_pcm, max_count * C, (max_count + m) * C, sent16), (big_taps, 8 * T, (8 + L) * T, sentd)):
        assert bool((bigt[:lo] == sent).all()) and bool((bigt[hi:] == sent).all())
    assert torch.equal(in_ring, before) and bool(torch.isfinite(out_ring).all())
    assert bool((out_ring.abs() < 1.5).all())           # every tap row came from the table, none from the sentinel rows
    # the first segment is a legitimate one but for its stream and its tap row: stream 0, outputs 5 .. 5 + 255 from r0 = 3
    J = (T - 2) // 2
    x = torch.cat([torch.zeros(J + 40, dtype=torch.float64), before[0].cpu()[100:300],      # slots 100 .. 299 are k = 0 .. 199,
                   torch.zeros(max_count * M // L + T, dtype=torch.float64)])               # zero below and, by hi, above
    num = 3 + np.arange(max_count) * M
    want = torch.stack([(x[40 + q:40 + q + T] * torch.from_numpy(taps_h[r])).sum() for q, r in zip(num // L, num % L)])
    assert torch.allclose(out_ring[0, 5:5 + max_count].cpu(), want, rtol=0, atol=1e-12)
    assert float(want.abs().max()) > 1e-3
